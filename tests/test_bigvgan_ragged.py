"""CPU: the ragged BigVGAN pass is declared, exported and bound; its packed layout (f5_bigvgan_ragged_plan, pure host arithmetic)
keeps consecutive items at least the convolutions' reach apart and refuses what the C ABI says it refuses; forward_ragged
validates its arguments without a device; and only the `.ragged()` view, not BigVGAN itself, has `decode_ragged`."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import ROOT

import f5_tts_amd as P
from f5_tts_amd import _lib

F5_OK, F5_EINVAL = 0, -1
NAMES = ("f5_bigvgan_forward_ragged", "f5_bigvgan_ragged_plan")
HALO = 25     # max (k - 1) / 2 * d over resblock kernels (3, 7, 11) x dilations (1, 3, 5)
FRAMES = (1, 2, 37, 5)


def test_ragged_entry_points_are_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "f5_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), f"{name} is not declared in include/f5_hip.h"
        assert hasattr(_lib.load(), name), f"{name} is not exported by libf5hip.so"
    res, args = _lib.SIGNATURES["f5_bigvgan_forward_ragged"]
    # (v, mel, B, stride_b, stride_c, stride_t, starts_host, ends_host, gain_host, wav, wav_stride, stream): f5_vocos_decode_ragged's
    assert (res, args) == _lib.SIGNATURES["f5_vocos_decode_ragged"]
    res, args = _lib.SIGNATURES["f5_bigvgan_ragged_plan"]
    assert res is C.c_int32 and len(args) == 5 and args[2:] == [C.POINTER(C.c_int32)] * 3


@pytest.mark.parametrize("cfg_name", ["BIGVGAN_TINY", "BIGVGAN_V2_24K"])
def test_plan_layout(cfg_name):
    cfg = getattr(P.config, cfg_name)
    bv = P.BigVGAN(cfg)
    rs, gap = bv.ragged_plan(FRAMES)
    assert len(rs) == len(FRAMES) + 1 and rs[0] == 0
    assert all(b > a for a, b in zip(rs, rs[1:])), "row_start is increasing"
    assert gap * cfg["upsample_rates"][0] >= HALO
    for b in range(len(FRAMES) - 1):
        assert rs[b + 1] - (rs[b] + FRAMES[b]) >= gap, f"items {b} and {b + 1} are less than the gap apart"
        assert rs[b + 1] * cfg["upsample_rates"][0] % 8 == 0, "an item starts on a tile of the activation kernel"
    assert rs[-1] == rs[-2] + FRAMES[-1], "row_start[B] is the packed frame count"
    # one item: the packed axis is the item
    assert bv.ragged_plan([9]) == ([0, 9], gap)


def test_plan_refusals():
    lib = _lib.load()
    bv = P.BigVGAN(P.config.BIGVGAN_V2_24K)
    cfg = bv._config()
    rs, gap = (C.c_int32 * 70000)(), C.c_int32()

    def plan(c, B, frames, rs_, gap_):
        code = lib.f5_bigvgan_ragged_plan(c, B, None if frames is None else _lib.int_array(frames), rs_, gap_)
        return code, lib.f5_last_error().decode()

    assert plan(C.byref(cfg), 2, [3, 4], rs, C.byref(gap))[0] == F5_OK
    for args in ((None, 2, [3, 4], rs, C.byref(gap)), (C.byref(cfg), 2, None, rs, C.byref(gap)),
                 (C.byref(cfg), 2, [3, 4], None, C.byref(gap)), (C.byref(cfg), 2, [3, 4], rs, None)):
        code, msg = plan(*args)
        assert code == F5_EINVAL and "null" in msg
    for B in (0, -1, 65536):
        code, msg = plan(C.byref(cfg), B, [3] * max(B, 1), rs, C.byref(gap))
        assert code == F5_EINVAL and f"B = {B}" in msg
    for bad in (0, -2):
        code, msg = plan(C.byref(cfg), 3, [3, 4, bad], rs, C.byref(gap))
        assert code == F5_EINVAL and "item 2" in msg
    # 2^24 rows at the last stage = 65,536 frames of the 256x generator
    assert plan(C.byref(cfg), 1, [65536], rs, C.byref(gap))[0] == F5_OK
    code, msg = plan(C.byref(cfg), 2, [40000, 30000], rs, C.byref(gap))
    assert code == F5_EINVAL and "2^24" in msg and "item 1" in msg


def test_null_handle_is_refused_without_a_device():
    lib = _lib.load()
    assert lib.f5_bigvgan_forward_ragged(None, None, 1, 0, 0, 0, None, _lib.int_array([4]), None, None, 0, None) == F5_EINVAL
    assert b"f5_bigvgan_forward_ragged" in lib.f5_last_error()


def test_forward_ragged_argument_errors_without_a_device():
    bv = P.BigVGAN(P.config.BIGVGAN_TINY).init_synthetic()
    mel = torch.zeros(2, 100, 8)
    for kw in (dict(ends=[8]), dict(ends=[8, 5], starts=[0]), dict(ends=[8, 5], gain=[1.0]),          # one entry per row
               dict(ends=[8, 9]), dict(ends=[8, 5], starts=[0, -1]), dict(ends=[8, 5], starts=[0, 5]),  # end > T, start < 0, no frame
               dict(ends=[8, 5], max_frames=0)):
        with pytest.raises(ValueError, match="forward_ragged"):
            bv.forward_ragged(mel, **kw)
    with pytest.raises(ValueError, match="forward_ragged"):
        bv.forward_ragged(torch.zeros(2, 80, 8), ends=[8, 5])
    # valid arguments reach the handle, which has no CPU path (the message of the plain forward)
    with pytest.raises(RuntimeError, match="only runs on a GPU") as ragged:
        bv.forward_ragged(mel, ends=[8, 5], starts=[0, 4])      # a one-frame item is allowed
    with pytest.raises(RuntimeError) as plain:
        bv(mel)
    assert str(ragged.value) == str(plain.value)


def test_max_frames_groups_are_consecutive_and_bounded():
    bv = P.BigVGAN(P.config.BIGVGAN_TINY)
    frames = [33, 1, 130, 64, 5, 5]
    assert bv._ragged_groups(frames, None) == [range(6)]
    groups = bv._ragged_groups(frames, 100)
    assert [i for g in groups for i in g] == list(range(6)) and len(groups) > 1
    for g in groups:
        rs, _ = bv.ragged_plan(frames[g.start:g.stop])
        assert rs[-1] <= 100 or len(g) == 1, "only an item longer than max_frames exceeds it, alone"
    assert range(2, 3) in groups      # 130 frames > 100


def test_only_the_view_has_decode_ragged():
    bv = P.BigVGAN(P.config.BIGVGAN_TINY)
    assert hasattr(bv, "decode_ragged") is False
    view = bv.ragged()
    assert hasattr(view, "decode_ragged") is True
    assert view.vocoder is bv and view.total_up == bv.total_up == 8 and view.cfg is bv.cfg
    with pytest.raises(NotImplementedError, match=r"ragged\(\)"):
        P.infer.synthesize_batch(None, bv, torch.zeros(1, 4, 100), torch.ones(1, 3, dtype=torch.long), 9, lens=[4])
