"""GPU: the argument rules the four sampler entry points share (f5_sample, f5_sample_ode, f5_sample_items, f5_sample_span), one
table of mistakes applied to each through ctypes.  A refused call returns F5_EINVAL, says which entry point refused it, and
enqueues nothing: both outputs keep their sentinel.  F5TTS_TINY, f32, B = 2, N = 8, nt = 4, 2 steps."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import DEV, SENT32, Guarded, _a, _p, _s  # noqa: E402

import f5_tts_amd as P  # noqa: E402
from f5_tts_amd import _lib  # noqa: E402

F5_OK, F5_EINVAL = 0, -1
B, N, NT, STEPS, MEL, REF = 2, 8, 4, 2, 100, 3
ENTRY_POINTS = ("f5_sample", "f5_sample_ode", "f5_sample_items", "f5_sample_span")
# what a caller can get wrong in the arguments every entry point has
MISTAKES = {"lens missing with B = 2": dict(lens=None),
            "lens[1] = 0": dict(lens=[N, 0]),
            "lens[0] = N + 1": dict(lens=[N + 1, N]),
            "cond_frames = N + 1": dict(cond_frames=N + 1),
            "nt = 0": dict(nt=0),
            "null out": dict(out=None),
            "null cond_mask": dict(mask=None)}


def good_args():
    """A call every entry point accepts.  (cond holds N + 1 frames, so that no row of the table names memory that is not there.)"""
    g = torch.Generator().manual_seed(11)
    mask = torch.zeros(B, N, dtype=torch.uint8)
    mask[:, :REF] = 1
    return dict(cond=torch.randn(B, N + 1, MEL, generator=g).to(DEV), cond_frames=REF, mask=mask.to(DEV),
                y0=torch.randn(B, N, MEL, generator=g).to(DEV), text=torch.randint(0, 39, (B, NT), generator=g).to(DEV), nt=NT,
                lens=[N, 5], out=Guarded((B, N, MEL), torch.float32))


def call(lib, h, name, a, second):
    """`name` with the arguments a; second: the trajectory (STEPS + 1 slots) or, for f5_sample_span, the state."""
    t = [0.0, 0.5, 1.0]
    grid, grids, steps, cfgs = _lib.float_array(t), _lib.float_array(t * B), _lib.int_array([STEPS] * B), _lib.float_array([2.0] * B)
    head = (h, _p(a["cond"]), a["cond_frames"], _p(a["mask"]))
    tail = (_lib.int_array(a["lens"]), B, N, _a(a["out"]), _a(second), _s())
    if name == "f5_sample":
        return lib.f5_sample(*head, _p(a["y0"]), _p(a["text"]), a["nt"], grid, STEPS, 2.0, *tail)
    if name == "f5_sample_ode":
        return lib.f5_sample_ode(*head, _p(a["y0"]), _p(a["text"]), a["nt"], grid, STEPS, 2.0, *tail, 0)
    if name == "f5_sample_items":
        return lib.f5_sample_items(*head, _p(a["y0"]), _p(a["text"]), a["nt"], grids, steps, STEPS, cfgs, *tail, 0)
    return lib.f5_sample_span(*head, _p(a["y0"]), None, 0, 0, _lib.int_array([-1] * B), _p(a["text"]), a["nt"], grids, steps, STEPS, cfgs,
                              *tail, 0)


def second_output(name):
    return Guarded((B, N, MEL) if name == "f5_sample_span" else (STEPS + 1, B, N, MEL), torch.float32)


@pytest.fixture(scope="module")
def engine():
    tr = P.DiT(**P.config.F5TTS_TINY, text_num_embeds=40, mel_dim=MEL, precision="f32").init_synthetic(seed=2).to(DEV)
    return tr.engine()


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_shared_mistakes_are_refused_by_name_and_write_nothing(engine, name):
    lib = engine.lib
    with torch.cuda.device(DEV):
        for what, wrong in MISTAKES.items():
            a, second = good_args(), second_output(name)
            out = a["out"]
            a.update(wrong)
            rc = call(lib, engine._h, name, a, second)
            msg = lib.f5_last_error()
            assert rc == F5_EINVAL, f"{name}, {what}: rc {rc}, {msg}"
            assert msg.startswith(name.encode() + b":"), f"{name}, {what}: the message does not begin with the entry point's name: {msg}"
            torch.cuda.synchronize()
            for buf in (out, second):
                assert bool((buf.bits == SENT32).all()) and buf.guards_intact(), f"{name}, {what}: a refused call wrote an output"
        # the table's starting point is a call that runs
        a, second = good_args(), second_output(name)
        assert call(lib, engine._h, name, a, second) == F5_OK, lib.f5_last_error()
        torch.cuda.synchronize()
        assert torch.isfinite(a["out"].value).all() and torch.isfinite(second.value).all()
        assert a["out"].guards_intact() and second.guards_intact()
