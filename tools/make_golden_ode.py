"""Generates the midpoint-solver fixtures tests/golden/sample_*_midpoint*.npz by RUNNING THE REFERENCE.

    python tools/make_golden_ode.py [name ...]

Build container only (the reference never travels to the GPU box).  The reference's CFM is loaded through
oracle.ref_harness; its `odeint` (torchdiffeq, not installed) is rebound to the fixed-grid stand-in of
tests/ode_oracle.py, which adds torchdiffeq's midpoint rule, and the model is switched to it exactly as a user does:
`model.odeint_kwargs = dict(method="midpoint")`.  Weights, inputs, meta and file format are those of
oracle/make_golden.py (build / save are reused), plus two meta keys:
  method          "midpoint"
  time_mlp_scale  factor applied to both time-MLP weight matrices after the synthetic draw (every consumer applies it:
                  tests/ode_oracle.py::scaled_time_mlp).  With the N(0, 0.02^2) synthetic weights the time embedding
                  barely moves the velocity, so a midpoint solve evaluated at the wrong time would be indistinguishable
                  from the right one; the factor makes the fixtures sensitive to the evaluation times.
"""
from __future__ import annotations

import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

_argv, sys.argv = sys.argv, sys.argv[:1]   # oracle.make_golden reads its fixture filter from sys.argv at import
try:
    from oracle import make_golden as mg  # noqa: E402
finally:
    sys.argv = _argv

import f5_tts_amd as P  # noqa: E402
import ode_oracle  # noqa: E402
from oracle import ref_harness as rh  # noqa: E402

TIME_MLP_SCALE = 8.0
TINY = dict(P.config.F5TTS_TINY)
E2_TINY = dict(dim=256, depth=4, heads=4, dim_head=64, ff_mult=2, text_mask_padding=False, pe_attn_head=1,
               text_dim=None, conv_layers=0, attn_mask_enabled=False, qk_norm=None)

# name -> sample_case keywords (the keywords of oracle/make_golden.py::sample_case)
CASES = {
    "sample_b1_midpoint": dict(arch=TINY, B=1, cond_len=24, nt=14, duration=64, steps=16),
    # attn_mask_enabled ragged batch: the engine runs it on packed rows (RowPack half-step kernel)
    "sample_b3_midpoint_attnmask": dict(arch=dict(TINY, attn_mask_enabled=True), B=3, cond_len=18, nt=12,
                                        duration=[44, 27, 35], lens=[18, 11, 14], steps=8, use_epss=False,
                                        text_pad=[12, 7, 9]),
    # single conditional forward per evaluation; the solve starts at t_inter (steps -> int(10 * 0.8) = 8)
    "sample_b1_midpoint_nocfg": dict(arch=TINY, B=1, cond_len=18, nt=9, duration=52, steps=10, cfg_strength=0.0,
                                     sway=None, duplicate_test=True, t_inter=0.2),
    "sample_unett_b2_midpoint": dict(arch=E2_TINY, B=2, cond_len=20, nt=12, duration=[44, 31], lens=[20, 12], steps=6,
                                     text_pad=[12, 8], backbone="UNetT"),
}


def generate(name):
    """Runs the reference for one fixture; returns (meta, arrays) exactly as they are saved."""
    k = dict(CASES[name])
    arch, B, backbone = k.pop("arch"), k.pop("B"), k.pop("backbone", "DiT")
    cond_len, nt, duration, steps = k.pop("cond_len"), k.pop("nt"), k.pop("duration"), k.pop("steps")
    lens, text_pad = k.pop("lens", None), k.pop("text_pad", None)
    cfg_strength, sway, seed = k.pop("cfg_strength", 2.0), k.pop("sway", -1.0), k.pop("seed", 7)
    use_epss, duplicate_test, t_inter = k.pop("use_epss", True), k.pop("duplicate_test", False), k.pop("t_inter", 0.1)
    assert not k, k
    ref = rh.load()
    ref.cfm.odeint = ode_oracle.reference_odeint
    model, sd = mg.build(arch, backbone, 0)
    model.transformer.load_state_dict(ode_oracle.scaled_time_mlp(sd, TIME_MLP_SCALE), strict=True)
    model.odeint_kwargs = dict(method="midpoint")
    g = torch.Generator().manual_seed(1000 + len(name))
    cond = torch.randn(B, cond_len, 100, generator=g)
    text = torch.randint(0, mg.NVOCAB, (B, nt), generator=g)
    if text_pad:
        for b, n_valid in enumerate(text_pad):
            text[b, n_valid:] = -1
    kw = dict(steps=steps, cfg_strength=cfg_strength, sway_sampling_coef=sway, seed=seed, use_epss=use_epss)
    if lens is not None:
        kw["lens"] = torch.tensor(lens)
    if duplicate_test:
        kw.update(duplicate_test=True, t_inter=t_inter)
    with torch.no_grad():
        out, traj = model.sample(cond, text, duration if isinstance(duration, int) else torch.tensor(duration), **kw)
    meta = dict(arch=arch, backbone=backbone, nvocab=mg.NVOCAB, wseed=0, steps=steps, cfg_strength=cfg_strength,
                sway=sway, seed=seed, use_epss=use_epss, no_ref_audio=False, duration=duration, lens=lens,
                weights_checksum=mg.weights_checksum(sd), duplicate_test=duplicate_test, t_inter=t_inter,
                method="midpoint", time_mlp_scale=TIME_MLP_SCALE)
    return meta, dict(cond=cond, text=text, out=out, traj=traj)


def main(names):
    for name in names or CASES:
        meta, arrays = generate(name)
        mg.save(name, meta, **arrays)


if __name__ == "__main__":
    main(sys.argv[1:])
