"""Generates tests/golden/mmdit_*.npz by RUNNING THE REFERENCE's MMDiT (imported where it lies through oracle/ref_harness.py).

    python tools/make_mmdit_golden.py [fixture names ...]

Runs only where the reference tree is present.  Every output tensor comes from the reference's own code (cfm.py, backbones/mmdit.py,
modules.py); inputs and the synthetic-weight recipe (seed, std) are recorded beside them.  Weights are NOT stored: they are regenerated
from (seed, tensor name) by weights.synthetic_state_dict, and a checksum detects generator drift.

Weight scale.  At the project's usual std = 0.02 the text stream hardly reaches the output (swapping a token moves `out` by ~2e-5,
far inside the 1e-3 parity bar: an engine that ignored the text stream would pass).  The fixtures therefore use STD below -- the
smallest hundredth at which every fixture clears the condition with margin (measured on the reference at these shapes, one token /
reversed order: 0.04 1.3e-2 / 1.4e-2, 0.05 4.2e-2 / 5.6e-2, 0.06 1.2e-1 / 2.0e-1, 0.07 4.9e-1 / 6.3e-1, 0.1 6.7 / 9.0: beyond 0.06 the
model only gets more chaotic) -- and the generator asserts on the reference, for every `sample` fixture, that replacing one token of item 0 and reversing item 0's valid
tokens each move `out` by at least SENSITIVITY = 2e-2 (20 x the parity bar).  Both perturbed outputs are stored (out_token,
out_order) so that a CPU test re-asserts the condition without the reference.
"""
from __future__ import annotations

import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import f5_tts_amd as P  # noqa: E402
from oracle import ref_harness as rh  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
NVOCAB = 40
STD = 0.06
SENSITIVITY = 2e-2
ARCH = dict(dim=256, depth=3, heads=4, dim_head=64, ff_mult=2, text_mask_padding=True, qk_norm=None)
ONLY = set(sys.argv[1:])


def weights_checksum(sd):
    return float(sum(v.double().abs().sum().item() for v in sd.values()))


def save(name, meta, **arrays):
    arrs = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in arrays.items()}
    arrs["meta_json"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **arrs)
    print("wrote", name, {k: v.shape for k, v in arrs.items() if k != "meta_json"})


def build(arch, wseed=0):
    ref = rh.load()
    mmdit = importlib.import_module("f5_tts.model.backbones.mmdit")
    sd = P.weights.synthetic_state_dict(P.weights.mmdit_param_shapes(arch, NVOCAB), seed=wseed, std=STD)
    tr = mmdit.MMDiT(**arch, text_num_embeds=NVOCAB, mel_dim=100)
    model = ref.CFM(transformer=tr, mel_spec_module=rh.InertMelSpec()).eval()
    tr.load_state_dict(sd, strict=True)
    return model, sd


def case_inputs(name, B, cond_len, nt, text_valid):
    g = torch.Generator().manual_seed(2000 + len(name))
    cond = torch.randn(B, cond_len, 100, generator=g)
    text = torch.randint(0, NVOCAB, (B, nt), generator=g)
    for b, n_valid in enumerate(text_valid or []):
        text[b, n_valid:] = -1
    return cond, text


def perturbed_texts(text):
    """Item 0 with its first token replaced, and item 0 with its valid tokens in reverse order."""
    n0 = int((text[0] != -1).sum())
    tok = text.clone()
    tok[0, 0] = (tok[0, 0] + 1 + NVOCAB // 2) % NVOCAB
    order = text.clone()
    order[0, :n0] = text[0, :n0].flip(0)
    assert not torch.equal(order, text), "item 0's tokens read the same in both directions: draw another text"
    return tok, order


def sample_case(name, arch, *, B, cond_len, nt, duration, lens=None, text_valid=None, steps, cfg_strength=2.0, sway=-1.0, seed=7,
                use_epss=True, edit_mask=None):
    if ONLY and name not in ONLY:
        return
    model, sd = build(arch)
    cond, text = case_inputs(name, B, cond_len, nt, text_valid)
    kw = dict(steps=steps, cfg_strength=cfg_strength, sway_sampling_coef=sway, seed=seed, use_epss=use_epss)
    if lens is not None:
        kw["lens"] = torch.tensor(lens)
    if edit_mask is not None:
        kw["edit_mask"] = edit_mask
    dur = duration if isinstance(duration, int) else torch.tensor(duration)
    out, traj = model.sample(cond, text, dur, **kw)
    tok, order = perturbed_texts(text)
    out_token, _ = model.sample(cond, tok, dur, **kw)
    out_order, _ = model.sample(cond, order, dur, **kw)
    d_tok, d_ord = float((out_token - out).abs().max()), float((out_order - out).abs().max())
    print(f"{name}: |out| <= {float(out.abs().max()):.3f}; one token moves out by {d_tok:.3e}, reversed order by {d_ord:.3e}")
    assert d_tok >= SENSITIVITY and d_ord >= SENSITIVITY, f"{name}: the text stream does not reach the output at std={STD}"
    meta = dict(arch=arch, backbone="MMDiT", nvocab=NVOCAB, wseed=0, std=STD, steps=steps, cfg_strength=cfg_strength, sway=sway, seed=seed,
                use_epss=use_epss, duration=duration, lens=lens, weights_checksum=weights_checksum(sd), sensitivity=SENSITIVITY,
                moved_token=d_tok, moved_order=d_ord)
    arrays = dict(cond=cond, text=text, out=out, traj=traj, text_token=tok, text_order=order, out_token=out_token, out_order=out_order)
    if edit_mask is not None:
        arrays["edit_mask"] = edit_mask
    save(name, meta, **arrays)


def forward_taps_case(name, arch, *, B, N, nt, durations, text_valid):
    """One forward of the ragged case (cfg_infer: cond and uncond halves packed) with taps taken by forward hooks."""
    if ONLY and name not in ONLY:
        return
    model, sd = build(arch)
    tr = model.transformer
    g = torch.Generator().manual_seed(77)
    x = torch.randn(B, N, 100, generator=g)
    cond = torch.randn(B, N, 100, generator=g)
    cond[:, N // 3:] = 0
    text = torch.randint(0, NVOCAB, (B, nt), generator=g)
    for b, n_valid in enumerate(text_valid):
        text[b, n_valid:] = -1
    time = torch.tensor(0.3)
    mask = torch.arange(N)[None] < torch.tensor(durations)[:, None]
    taps = {}

    def hook(key, both=False):
        def f(mod, inp, out):
            if both:   # MMDiTBlock returns (c, x); the last block's c is None
                if out[0] is not None:
                    taps[key + "_c"] = out[0].detach().clone()
                taps[key + "_x"] = out[1].detach().clone()
            else:
                taps.setdefault(key, []).append(out.detach().clone())
        return f

    hs = [tr.audio_embed.register_forward_hook(hook("audio_embed"))]
    for i, blk in enumerate(tr.transformer_blocks):
        hs.append(blk.register_forward_hook(hook(f"block{i}", both=True)))
    with torch.no_grad():
        out = tr(x=x, cond=cond, text=text, time=time, mask=mask, cfg_infer=True, cache=True)
        taps["text_cond"] = tr.text_cond.clone()
        taps["text_uncond"] = tr.text_uncond.clone()
        tr.clear_cache()
    for h in hs:
        h.remove()
    taps["audio_embed"] = torch.cat(taps["audio_embed"], dim=0)   # the cond call, then the uncond call: [2 B, N, D]
    meta = dict(arch=arch, backbone="MMDiT", nvocab=NVOCAB, wseed=0, std=STD, weights_checksum=weights_checksum(sd), durations=durations)
    # three files, each under the repository's size limit for one file: inputs, output and the text stream; then the audio stream
    xs = {k: taps.pop(k) for k in list(taps) if k.endswith("_x")}
    ae = taps.pop("audio_embed")
    nb = len(tr.transformer_blocks)
    save(name, meta, x=x, cond=cond, text=text, time=time, mask=mask, out=out, **taps)
    save(name + "_x0", meta, audio_embed=ae, **{k: v for k, v in xs.items() if int(k[5:-2]) < nb // 2})
    save(name + "_x1", meta, **{k: v for k, v in xs.items() if int(k[5:-2]) >= nb // 2})


def main():
    if not rh.available():
        raise SystemExit("the reference tree is not present: the fixtures cannot be generated here")
    sample_case("mmdit_b1_nfe4", ARCH, B=1, cond_len=24, nt=11, duration=50, steps=4)
    sample_case("mmdit_b3_ragged", ARCH, B=3, cond_len=24, nt=13, duration=[64, 37, 50], lens=[24, 17, 9], text_valid=[13, 6, 9], steps=4)
    sample_case("mmdit_b2_qknorm", dict(ARCH, depth=2, qk_norm="rms_norm", text_mask_padding=False), B=2, cond_len=20, nt=8,
                duration=[48, 48], lens=[20, 16], steps=4)
    em = torch.ones(1, 24, dtype=torch.bool)
    em[0, 8:15] = False
    sample_case("mmdit_b1_nocfg", ARCH, B=1, cond_len=24, nt=11, duration=50, steps=3, cfg_strength=0.0, use_epss=False, edit_mask=em)
    forward_taps_case("mmdit_forward_taps", ARCH, B=3, N=64, nt=13, durations=[64, 37, 50], text_valid=[13, 6, 9])


if __name__ == "__main__":
    main()
