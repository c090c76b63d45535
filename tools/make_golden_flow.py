"""Generates the flow-loss fixtures tests/golden/flow_loss_*.npz by RUNNING THE REFERENCE's CFM.forward on the CPU.

    python tools/make_golden_flow.py [name ...]

Build container only (the reference never travels to the GPU box).  The reference's CFM is loaded through oracle.ref_harness
(the MMDiT through tools/make_mmdit_golden.py's build); weights, meta and file format are those of tools/make_golden_ode.py:
synthetic weights regenerated from (seed, tensor name), the time MLP scaled by `time_mlp_scale` for the DiT and the UNetT and the
MMDiT's weights drawn at that tool's std, so that the time and the text reach the prediction -- the generator asserts on the
reference that another row's time and a reversed text each move `pred` by at least SENSITIVITY.

A case seeds torch and `random` with meta["seed"] and calls model.forward(inp, text, lens=lens).  The drop flags are forced through
the model's own probabilities (meta["audio_drop_prob"], meta["cond_drop_prob"]: 0.0 or 1.0).  The draws are recorded by replaying
them after the same seeding with the reference's own calls in the reference's order (cfm.py:261-291), and checked against what the
reference's transformer was handed (x, cond, time and the flags, captured by a forward pre-hook): span, x0, time, flags.
The mel `inp` is random outside the masked span and close to the fixed point x1 = x0 + pred(x1) inside it (see generate), so that
the loss is small, as a trained model's is, and reacts to every input of the glue.
Stored: inp, text, lens, the draws, and the reference's loss, cond and pred.
"""
from __future__ import annotations

import os
import random
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

_argv, sys.argv = sys.argv, sys.argv[:1]   # oracle.make_golden and make_mmdit_golden read fixture filters from sys.argv at import
try:
    from oracle import make_golden as mg  # noqa: E402
    import make_mmdit_golden as mm  # noqa: E402
finally:
    sys.argv = _argv

import f5_tts_amd as P  # noqa: E402
import ode_oracle  # noqa: E402
from oracle import ref_harness as rh  # noqa: E402

TIME_MLP_SCALE = 8.0
SENSITIVITY = 2e-2
FIXED_POINT_ITERS = 3   # (one more round takes the DiT's loss down to f32 rounding, where it says nothing)
TINY = dict(P.config.F5TTS_TINY)
E2_TINY = dict(dim=256, depth=4, heads=4, dim_head=64, ff_mult=2, text_mask_padding=False, pe_attn_head=1,
               text_dim=None, conv_layers=0, attn_mask_enabled=False, qk_norm=None)

# name -> case keywords; lens[0] is the padded length N
CASES = {
    "flow_loss_dit_b3": dict(arch=TINY, lens=[40, 33, 21], nt=12, text_pad=[12, 7, 9]),
    "flow_loss_dit_b2_drop_audio": dict(arch=TINY, lens=[36, 28], nt=10, text_pad=[10, 6], audio_drop_prob=1.0),
    "flow_loss_dit_b2_drop_both": dict(arch=TINY, lens=[36, 28], nt=10, text_pad=[10, 6], cond_drop_prob=1.0),
    "flow_loss_dit_b3_attnmask": dict(arch=dict(TINY, attn_mask_enabled=True), lens=[40, 33, 21], nt=12, text_pad=[12, 7, 9]),
    # (seed 7: the two rows draw times 0.85 and 0.05 -- the UNetT, whose time is one token, hardly tells 0.47 from 0.43)
    "flow_loss_unett_b2": dict(arch=E2_TINY, backbone="UNetT", lens=[36, 29], nt=12, text_pad=[12, 8], seed=7),
    "flow_loss_mmdit_b2": dict(arch=mm.ARCH, backbone="MMDiT", lens=[32, 25], nt=11, text_pad=[11, 7]),
}


def build(arch, backbone):
    """(reference CFM, synthetic state dict, meta entries of the weight recipe)"""
    if backbone == "MMDiT":
        model, sd = mm.build(arch)
        return model, sd, dict(std=mm.STD, time_mlp_scale=1.0)
    model, sd = mg.build(arch, backbone, 0)
    model.transformer.load_state_dict(ode_oracle.scaled_time_mlp(sd, TIME_MLP_SCALE), strict=True)
    return model, sd, dict(time_mlp_scale=TIME_MLP_SCALE)


def generate(name):
    k = dict(CASES[name])
    arch, backbone, lens, nt = k.pop("arch"), k.pop("backbone", "DiT"), k.pop("lens"), k.pop("nt")
    text_pad, seed = k.pop("text_pad"), k.pop("seed", 11)
    p_audio, p_cond = k.pop("audio_drop_prob", 0.0), k.pop("cond_drop_prob", 0.0)
    assert not k, k
    ref = rh.load()
    model, sd, recipe = build(arch, backbone)
    model.audio_drop_prob, model.cond_drop_prob = p_audio, p_cond
    B, N = len(lens), max(lens)
    g = torch.Generator().manual_seed(3000 + len(name))
    inp = torch.randn(B, N, 100, generator=g)
    text = torch.randint(0, mg.NVOCAB, (B, nt), generator=g)
    for b, n_valid in enumerate(text_pad):
        text[b, n_valid:] = -1
    lens_t = torch.tensor(lens)

    # the draws, made with the reference's own calls in its order (cfm.py:261-291): they depend on the seed and the shapes alone
    def draws():
        torch.manual_seed(seed)
        random.seed(seed)
        frac = torch.zeros((B,)).float().uniform_(*model.frac_lengths_mask)
        span_mask = ref.utils.mask_from_frac_lengths(lens_t, frac) & ref.utils.lens_to_mask(lens_t, length=N)
        x0 = torch.randn_like(inp)
        time = torch.rand((B,), dtype=inp.dtype)
        drop_audio = random.random() < p_audio
        drop_text = False
        if random.random() < p_cond:
            drop_audio = drop_text = True
        return span_mask, x0, time, drop_audio, drop_text

    span_mask, x0, time, drop_audio, drop_text = draws()
    span = []
    for b in range(B):
        idx = span_mask[b].nonzero().flatten()
        s, e = (int(idx[0]), int(idx[-1]) + 1) if len(idx) else (0, 0)
        assert int(span_mask[b].sum()) == e - s, "the span is not one interval"
        span.append([s, e])
    t3 = time[:, None, None]
    mask = ref.utils.lens_to_mask(lens_t, length=N)

    def glue(x1):
        return (1 - t3) * x0 + t3 * x1, torch.where(span_mask[..., None], torch.zeros_like(x1), x1)

    # The target.  With a random mel the loss is the variance of x1 - x0 (about 2) whatever the model predicts, and no mistake in the
    # glue moves it by more than a percent.  A trained model's loss is small because its prediction follows the flow, so inside the
    # span the mel is moved towards the fixed point x1 = x0 + pred(x1) by FIXED_POINT_ITERS rounds (outside it the random mel
    # stays, so the loss also shows which frames were selected).
    with torch.no_grad():
        for _ in range(FIXED_POINT_ITERS):
            phi, c = glue(inp)
            p = model.transformer(x=phi, cond=c, text=text, time=time, drop_audio_cond=drop_audio, drop_text=drop_text, mask=mask)
            inp = torch.where(span_mask[..., None], x0 + p, inp)

    seen = {}
    hook = model.transformer.register_forward_pre_hook(lambda mod, a, kw: seen.update(kw), with_kwargs=True)
    torch.manual_seed(seed)
    random.seed(seed)
    with torch.no_grad():
        loss, cond, pred = model(inp, text, lens=lens_t)
    hook.remove()
    phi, c = glue(inp)
    assert torch.equal(seen["time"], time) and torch.equal(seen["x"], phi), "the replayed draws are not the reference's"
    assert torch.equal(seen["cond"], c) and torch.equal(cond, c)
    assert seen["drop_audio_cond"] == drop_audio and seen["drop_text"] == drop_text and torch.equal(seen["mask"], mask)

    # the fixture must be able to tell a wrong time and a wrong text from the right ones
    with torch.no_grad():
        kw = dict(x=seen["x"], cond=cond, drop_audio_cond=drop_audio, drop_text=drop_text, mask=seen["mask"])
        d_time = float((model.transformer(text=text, time=time.roll(1), **kw) - pred).abs().max())
        rev = text.clone()
        rev[0, :text_pad[0]] = text[0, :text_pad[0]].flip(0)
        d_text = float((model.transformer(text=rev, time=time, **kw) - pred).abs().max())
    print(f"{name}: loss {float(loss):.6f}, |pred| <= {float(pred.abs().max()):.3f}; another row's time moves pred by {d_time:.3e}, "
          f"a reversed text by {d_text:.3e}; span {span}, time {time.tolist()}, drops {drop_audio, drop_text}")
    assert d_time >= SENSITIVITY, f"{name}: the time does not reach the prediction"
    assert drop_text or d_text >= SENSITIVITY, f"{name}: the text does not reach the prediction"

    meta = dict(arch=arch, backbone=backbone, nvocab=mg.NVOCAB, wseed=0, seed=seed, lens=lens, audio_drop_prob=p_audio,
                cond_drop_prob=p_cond, drop_audio_cond=drop_audio, drop_text=drop_text, span=span, n_selected=int(span_mask.sum()) * 100,
                weights_checksum=mg.weights_checksum(sd), moved_time=d_time, moved_text=d_text, fixed_point_iters=FIXED_POINT_ITERS,
                **recipe)
    return meta, dict(inp=inp, text=text, x0=x0, time=time, loss=loss, cond=cond, pred=pred)


def main(names):
    if not rh.available():
        raise SystemExit("the reference tree is not present: the fixtures cannot be generated here")
    for name in names or CASES:
        meta, arrays = generate(name)
        mg.save(name, meta, **arrays)


if __name__ == "__main__":
    main(sys.argv[1:])
