"""Generates tests/golden/dit_exposed_forward.npz and tests/golden/unett_exposed_forward.npz by RUNNING THE REFERENCE's DiT and UNetT
(imported where they lie through oracle/ref_harness.py) on the exposing weights of tests/backbone_cases.py.

    python tools/make_exposed_golden.py

Runs only where the reference tree is present.  The output tensor comes from the reference's own code (backbones/dit.py,
backbones/unett.py, modules.py): one cfg_infer forward of the [65, 37] case of each backbone, whose softmax is peaked and whose
AdaLN gates are about 0.5, so that tests/test_backbone_exposure.py's oracle is pinned against the reference itself where every block
counts.  Only the inputs, the output and the meta JSON are stored; the weights are regenerated from (seed, tensor name, factors) by
backbone_cases.exposing_weights, and a checksum detects generator drift.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import backbone_cases as BC  # noqa: E402
from oracle import ref_harness as rh  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
FIXTURES = {"dit_exposed_forward": "dit_b2", "unett_exposed_forward": "unett_b2"}


def save(name, meta, **arrays):
    arrs = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in arrays.items()}
    arrs["meta_json"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **arrs)
    print("wrote", name, {k: v.shape for k, v in arrs.items() if k != "meta_json"})


def forward_case(name, case_name):
    c = BC.CASE[case_name]
    sd = BC.weights_for(c.key)
    model = rh.build_reference_cfm(dict(c.arch), BC.NV, backbone=c.backbone)
    tr = model.transformer
    tr.load_state_dict(sd, strict=True)
    x, cond, text, time, mask = BC.inputs(case_name)
    with torch.no_grad():
        out = tr(x=x, cond=cond, text=text, time=time, mask=mask, cfg_infer=True, cache=True)
        tr.clear_cache()
    e = BC.linf(out, BC.reference(case_name), BC.valid(case_name))
    print(f"{name}: |out| <= {float(out.abs().max()):.3f}; the reference (float32) is {e:.3e} from the float64 oracle on valid frames")
    meta = dict(case=case_name, arch=c.arch, backbone=c.backbone, nvocab=BC.NV, wseed=BC.WSEED, factors=[[list(s), f] for s, f in BC.FACTORS[c.backbone]],
                lens=list(c.lens), weights_checksum=BC.weights_checksum(sd))
    save(name, meta, x=x, cond=cond, text=text, time=time, mask=mask, out=out)


def main():
    if not rh.available():
        raise SystemExit("the reference tree is not present: the fixtures cannot be generated here")
    for name, case_name in FIXTURES.items():
        forward_case(name, case_name)


if __name__ == "__main__":
    main()
