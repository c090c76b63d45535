"""GPU: the launches of one backbone forward, per class, for each of the three backbones -- the engine's per-launch profiler counts
them (one event pair per launch, eager).  sample() is run with 2 steps and with 3: the difference of the two `launches` dictionaries
is ONE step, i.e. one forward plus one Euler update (class misc); the time path and the text encoder run once per call, so their
difference is 0.  The expected numbers are a condition read off the stages of csrc/engine_impl.h (embed_input, the block loop of each
forward, finish), not a measurement: a stage that gains, loses or moves a launch fails here.

Per forward, d = depth:
  DiT     gemm 4d + 2 (4 per block, input and output projection), attention d, layernorm 2d + 1, convpos 2, misc 1 (input pack);
          qk_norm: misc + d (norm-rope);  long skip: gemm + 1, misc + 1 (concat);  f8: misc + 2d (the stand-alone row quantisers in
          front of the out-projection and FF2; the LayerNorms write the e4m3 operand of QKV and FF1 themselves)
  UNetT   gemm 4d + 2 + d/2 (skip projections of the upper half), attention d, layernorm 2d + 1, convpos 2,
          misc 3 + d/2 (pack, assemble, d/2 concats, strip)
  MMDiT   gemm 8(d - 1) + 5 + 2, attention d, layernorm 4(d - 1) + 3 + 1, convpos 2, misc 2 + d (pack, V^T zero, d splits);
          with lengths: misc + 1 (joint key lengths);  qk_norm: misc + 2d
          (= run_mmdit_forward's "launches per block": 14, or 10 in the last, context_pre_only block)"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import f5_tts_amd as P  # noqa: E402

DEV = "cuda:0"
N, NT, NV = 40, 8, 40
CLASSES = ("gemm", "attention", "layernorm", "convpos", "misc", "text_encoder", "time_adaln")


def dit_forward(d, qk_norm=False, long_skip=False, precision="f16"):
    return dict(gemm=4 * d + 2 + (1 if long_skip else 0), attention=d, layernorm=2 * d + 1, convpos=2,
                misc=1 + (d if qk_norm else 0) + (1 if long_skip else 0) + (2 * d if precision == "f8" else 0))


def unett_forward(d):
    return dict(gemm=4 * d + 2 + d // 2, attention=d, layernorm=2 * d + 1, convpos=2, misc=3 + d // 2)


def mmdit_forward(d, qk_norm=False, lens=False):
    return dict(gemm=8 * (d - 1) + 5 + 2, attention=d, layernorm=4 * (d - 1) + 3 + 1, convpos=2,
                misc=2 + d + (1 if lens else 0) + (2 * d if qk_norm else 0))


def one_step(tr, lens=None):
    """launches(3 steps) - launches(2 steps) of sample() without CFG, per profiler class."""
    eng = tr.to(DEV).engine()
    B = 1 if lens is None else len(lens)
    g = torch.Generator().manual_seed(5)
    cond = torch.randn(B, 12, 100, generator=g)
    cm = torch.zeros(B, N, dtype=torch.bool)
    cm[:, :12] = True
    y0 = torch.randn(B, N, 100, generator=g)
    text = torch.randint(0, NV, (B, NT), generator=g)
    counts = []
    for steps in (2, 3):
        eng.profile(True)   # (clears the counters)
        out, _ = eng.sample(cond, cm, y0, text, [i / steps for i in range(steps + 1)], 0.0, lens=lens, want_traj=False)
        prof = eng.profile_read()
        assert torch.isfinite(out).all()
        counts.append({k: prof[k]["launches"] for k in CLASSES})
    eng.profile(False)
    return {k: counts[1][k] - counts[0][k] for k in CLASSES}


def expect(forward):
    return dict(forward, misc=forward["misc"] + 1, text_encoder=0, time_adaln=0)   # + the step's Euler update


def arch(depth, **kw):
    return dict(dim=256, depth=depth, heads=4, dim_head=64, ff_mult=2, **kw)


@pytest.mark.parametrize("opts", [dict(), dict(qk_norm=True), dict(long_skip=True), dict(precision="f8")],
                         ids=["plain", "qk_norm", "long_skip", "f8"])
def test_dit_step_launches(opts):
    d = 2
    tr = P.DiT(**arch(d, qk_norm="rms_norm" if opts.get("qk_norm") else None, long_skip_connection=bool(opts.get("long_skip"))),
               text_num_embeds=NV, mel_dim=100, precision=opts.get("precision", "f16")).init_synthetic()
    assert one_step(tr) == expect(dit_forward(d, **opts))


def test_unett_step_launches():
    d = 4
    tr = P.UNetT(**arch(d), text_num_embeds=NV, mel_dim=100, precision="f16").init_synthetic()
    assert one_step(tr) == expect(unett_forward(d))


@pytest.mark.parametrize("qk_norm,lens", [(False, None), (False, [40, 29]), (True, None)], ids=["plain", "lens", "qk_norm"])
def test_mmdit_step_launches(qk_norm, lens):
    d = 3
    tr = P.MMDiT(**arch(d), qk_norm="rms_norm" if qk_norm else None, text_num_embeds=NV, mel_dim=100, precision="f16").init_synthetic()
    assert one_step(tr, lens) == expect(mmdit_forward(d, qk_norm=qk_norm, lens=lens is not None))
