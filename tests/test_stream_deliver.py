"""CPU: the delivery stage and the streaming session as far as they go without a device -- f5_wave_deliver_plan against
hand-computed cases and a brute-force count, every refusal of f5_wave_deliver decided before the first HIP call, the symbols
declared, exported and bound, the host text plan of a stream (stream_chunks) against hand-computed cases, and the session's
first-package state through plan() and reset()."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

import deliver_oracle as O

import f5_tts_amd as P
from f5_tts_amd import _lib
from f5_tts_amd import infer as I
from f5_tts_amd import stream as S

F5_EINVAL, F5_ESTATE = -1, -3
RATES = (24000, 16000, 8000, 22050, 44100, 48000)


def c_plan(out_rate, n, final):
    ln, ready = C.c_int64(-1), C.c_int64(-1)
    rc = _lib.load().f5_wave_deliver_plan(out_rate, n, int(final), C.byref(ln), C.byref(ready))
    return rc, ln.value, ready.value


def test_deliver_stage_is_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "f5_hip.h")).read()
    assert re.search(r"#define\s+F5_PCM_F32\s+0\b", src) and re.search(r"#define\s+F5_PCM_S16\s+1\b", src)
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _lib.load()
    for name, nargs in (("f5_wave_deliver_plan", 5), ("f5_wave_deliver", 14)):
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), f"{name} is not declared in include/f5_hip.h"
        assert hasattr(lib, name), f"{name} is not exported by libf5hip.so"
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int32 and len(args) == nargs
    assert (_lib.F5_PCM_F32, _lib.F5_PCM_S16) == (0, 1)
    for name in ("wave_deliver", "deliver_plan", "deliver_waves", "stream_chunks", "open_stream", "StreamSession"):
        assert hasattr(I, name), f"infer does not export {name}"
    assert "resampling of the OUTPUT" not in I.__doc__


def test_geometry_of_the_tested_rates():
    # (orig, new, width, K): width = ceil(6 orig / (0.99 min(orig, new)))
    assert O.geometry(24000) == (1, 1, 0, 1)
    assert O.geometry(16000) == (3, 2, 10, 23)           # 18 / 1.98 = 9.09
    assert O.geometry(8000) == (3, 1, 19, 41)            # 18 / 0.99 = 18.18
    assert O.geometry(48000) == (1, 2, 7, 15)            # 6 / 0.99 = 6.06
    assert O.geometry(22050) == (160, 147, 7, 174)       # 960 / 145.53 = 6.6
    assert O.geometry(44100) == (80, 147, 7, 94)         # 480 / 79.2 = 6.06
    assert O.geometry(192000) == (1, 8, 7, 15)


@pytest.mark.parametrize("out_rate, n, final, want", [
    (16000, 100, True, (67, 67)),            # ceil(200 / 3)
    (16000, 100, False, (67, 60)),           # floor(87 / 3) + 1 = 30 frames of 2
    (16000, 12, False, (8, 0)),              # floor(-1 / 3) = -1: no frame yet
    (16000, 13, False, (9, 2)),              # the first frame needs 10 + 3 samples
    (16000, 1, False, (1, 0)),
    (16000, 0, True, (0, 0)),
    (48000, 4097, False, (8194, 8180)),      # 4097 - 8 + 1 = 4090 frames of 2
    (8000, 22, False, (8, 1)),
    (8000, 21, False, (7, 0)),
    (24000, 5, False, (5, 5)),               # pass-through: every sample is settled at once
    (22050, 167, False, (154, 147)),         # ceil(147 * 167 / 160) = 154; one frame of 147
    (22050, 166, False, (153, 0)),
    (44100, 87, False, (160, 147)),
    (44100, 87, True, (160, 160)),
    (8000, 2**31 - 1, True, (715827883, 715827883)),
])
def test_plan_hand_computed(out_rate, n, final, want):
    assert c_plan(out_rate, n, final) == (0, *want)
    assert O.plan(out_rate, n, final) == want
    assert I.deliver_plan(out_rate, n, final) == want


@pytest.mark.parametrize("out_rate", RATES)
def test_plan_ready_equals_a_brute_force_count(out_rate):
    for n in list(range(0, 400)) + [4096, 4097, 5003]:
        rc, ln, ready = c_plan(out_rate, n, False)
        assert rc == 0 and ready == O.ready_by_count(out_rate, n) and (ln, ready) == O.plan(out_rate, n, False), (out_rate, n)
        assert c_plan(out_rate, n, True) == (0, ln, ln)


def test_plan_refusals():
    lib = _lib.load()

    def refused(rc, *words):
        msg = lib.f5_last_error()
        assert rc == F5_EINVAL and msg.startswith(b"f5_wave_deliver_plan:") and all(w in msg for w in words), (rc, msg)

    refused(c_plan(7999, 10, True)[0], b"out_rate", b"7999")
    refused(c_plan(192001, 10, True)[0], b"out_rate")
    refused(c_plan(0, 10, True)[0], b"out_rate")
    refused(c_plan(8001, 10, True)[0], b"8001", b"2^20")
    refused(c_plan(16000, -1, True)[0], b"n = -1")
    refused(c_plan(16000, 2**31, True)[0], b"n =")
    a = C.c_int64()
    refused(lib.f5_wave_deliver_plan(16000, 5, 1, None, C.byref(a)), b"len_out")
    refused(lib.f5_wave_deliver_plan(16000, 5, 1, C.byref(a), None), b"ready_out")
    assert c_plan(8000, 10, True)[0] == 0 and c_plan(192000, 10, True)[0] == 0


@pytest.fixture(scope="module")
def unloaded_handle():
    h = C.c_void_p()
    assert _lib.load().f5_mel_create(1024, 256, 100, C.byref(h)) == 0       # host bookkeeping only: no table, no bank
    return h


def test_deliver_refusals_without_a_device(unloaded_handle):
    """Every refusal is decided before the first HIP call; the pointers are never dereferenced on the way."""
    lib = _lib.load()
    h = unloaded_handle
    buf = (C.c_float * 4)()
    ptr = C.cast(buf, C.c_void_p)
    at = (C.c_int64 * 3)(-9, -9, -9)
    # three streams at 16 kHz: 100 final (67 ready), 100 growing (60 ready), 13 growing (2 ready): 67 | pad to 68 | 60 | 2 = 130 elements
    NS, FIN, O0, O1 = [100, 100, 13], [1, 0, 0], [0, 0, 0], [67, 60, 2]

    def call(m=h, base=ptr, B=3, starts=(0, 100, 200), n=NS, fin=FIN, o0=O0, o1=O1, rate=16000, fmt=0, out=ptr, cap=130, at_out=at):
        arr = lambda v: None if v is None else (C.c_int64 * len(v))(*v)   # noqa: E731
        return lib.f5_wave_deliver(m, base, B, arr(starts), _lib.int_array(n), _lib.int_array(fin), arr(o0), arr(o1), rate, fmt, out, cap,
                                   at_out, None)

    def refused(rc, *words):
        msg = lib.f5_last_error()
        assert rc == F5_EINVAL, (rc, msg)
        assert msg.startswith(b"f5_wave_deliver:") and all(w in msg for w in words), msg

    refused(call(m=None), b"m")
    refused(call(base=None), b"base")
    refused(call(starts=None), b"start_host")
    refused(call(n=None), b"n_host")
    refused(call(fin=None), b"final_host")
    refused(call(o0=None), b"o0_host")
    refused(call(o1=None), b"o1_host")
    refused(call(out=None), b"out")
    refused(call(at_out=None), b"out_start_out")
    refused(call(B=0), b"B")
    refused(call(B=-1), b"B")
    refused(call(B=65536), b"B")
    refused(call(rate=7999), b"out_rate")
    refused(call(rate=192001), b"out_rate")
    refused(call(rate=8001), b"8001", b"2^20")
    refused(call(fmt=2), b"format")
    refused(call(fmt=-1), b"format")
    refused(call(starts=(0, -1, 200)), b"item 1", b"start")
    refused(call(n=[100, 100, -1]), b"item 2", b"n = -1")
    refused(call(o1=[68, 60, 2]), b"item 0", b"ready = 67")           # past the end of a final stream
    refused(call(o1=[67, 61, 2]), b"item 1", b"ready = 60")           # a sample whose taps are not all there yet
    refused(call(o0=[0, 0, 3], o1=[67, 60, 2]), b"item 2")            # o0 > o1
    refused(call(o0=[-1, 0, 0]), b"item 0")
    refused(call(cap=129), b"out_capacity", b"130")
    refused(call(fmt=1, cap=137), b"out_capacity", b"138")            # s16 items start on multiples of 8: 67 | 72 + 60 | 136 + 2
    assert list(at) == [-9, -9, -9], "a refused call wrote out_start_out"
    # valid arguments: the only thing missing is the bank
    assert call() == F5_ESTATE and lib.f5_last_error().startswith(b"f5_wave_deliver:") and b"f5_mel_resample_bank" in lib.f5_last_error()
    assert list(at) == [-9, -9, -9]
    count = C.c_int32(-1)
    assert lib.f5_mel_resample_bank_count(h, C.byref(count)) == 0 and count.value == 0
    # empty ranges at the stream's own rate need no bank and launch nothing
    assert call(rate=24000, o1=[0, 0, 0], cap=0) == 0, lib.f5_last_error()
    assert list(at) == [0, 0, 0]


def test_python_wrappers_check_their_arguments_and_have_no_cpu_path():
    ms = P.mel.MelSpec()
    x = torch.zeros(100)
    with pytest.raises(RuntimeError, match="GPU"):
        I.wave_deliver(ms, [x], out_rate=16000)
    with pytest.raises(ValueError, match="sample_format"):
        I.wave_deliver(ms, [x], out_rate=16000, sample_format="u8")
    with pytest.raises(ValueError, match="no item"):
        I.wave_deliver(ms, [], out_rate=16000)
    with pytest.raises(ValueError, match="1-D f32"):
        I.wave_deliver(ms, [x[None]], out_rate=16000)
    with pytest.raises(ValueError, match="1-D f32"):
        I.wave_deliver(ms, [x[::2]], out_rate=16000)
    with pytest.raises(ValueError, match="one length per row"):
        I.deliver_waves(None, torch.zeros(2, 10), [10], out_rate=16000)
    with pytest.raises(_lib.F5Error, match="out_rate"):
        I.deliver_plan(7000, 10)


def test_the_oracle_quantiser_table():
    s = np.float32(32767.0)
    x = np.array([0.5, -0.5, 1.5, 2.5, 3.5], np.float32) / s
    x = np.concatenate([x, np.array([1.0, -1.0, 2.0, -2.0, np.inf, -np.inf, np.nan, 0.0, -32768.0 / 32767.0], np.float32)])
    t = x * s
    assert t[:5].tolist() == [0.5, -0.5, 1.5, 2.5, 3.5], "the table's ties are not exact in f32: the case lost its point"
    assert O.quantise(x).tolist() == [0, 0, 2, 2, 4, 32767, -32767, 32767, -32768, 32767, -32768, 0, 0, -32768]


# ------------------------------------------------------------------------------------------------ the host text plan
REF = "Some call me nature, others call me mother nature."    # 50 bytes
SENT = "The quick brown fox jumps over the lazy dog."           # 44 bytes


def test_stream_limits_hand_computed():
    # 50 bytes over 10 s = 5 bytes/s, times 15 s left of the 25: 75, then 37.5 and 18.75 truncated
    assert S.stream_limits(REF, 10.0) == (75, 37, 18)
    # 50 / 3 * 22 = 366.67: max 366, half 183.33 -> 183, a quarter 91.67 -> 91 (each truncated on its own, not 366 // 4)
    assert S.stream_limits(REF, 3.0) == (366, 183, 91)


def test_stream_chunks_hand_computed():
    text = " ".join([SENT] * 4)                                 # four sentences of 44 bytes
    # max_chars 75: a chunk holds one sentence (44 + 44 > 75)
    assert S.stream_chunks(text, REF, 10.0, first_package=False) == [SENT] * 4
    # first package: few_chars 37 and min_chars 18 are below one sentence, which has no inner punctuation: it stays whole
    assert S.stream_chunks(text, REF, 10.0, first_package=True) == [SENT] * 4
    # with commas the first chunk is cut down.  75: one sentence.  37: "Well, yes, of course, I said, " is 30 bytes and the 22 of
    # "it is a long way home." do not fit.  18: "Well, yes, " is 11 and "of course," (10) does not fit; "of course, " is 11 and
    # "I said," (7) just does
    first = "Well, yes, of course, I said, it is a long way home."  # 52 bytes
    got = S.stream_chunks(first + " " + SENT, REF, 10.0, first_package=True)
    assert got == ["Well, yes,", "of course, I said,", "it is a long way home.", SENT], got
    assert S.stream_chunks(first + " " + SENT, REF, 10.0, first_package=False) == [first, SENT]
    assert S.stream_chunks("", REF, 10.0, first_package=True) == [] and S.stream_chunks("", REF, 10.0, first_package=False) == []
    # a 3 s prompt: max 366 takes all four sentences (179 bytes) in one chunk; few 183 keeps it; min 91 splits it two and two
    assert S.stream_chunks(text, REF, 3.0, first_package=False) == [text]
    assert S.stream_chunks(text, REF, 3.0, first_package=True) == [SENT + " " + SENT] * 2


def test_packet_sizes_are_the_references_slicing():
    assert S.packet_sizes(5000, 2048) == [2048, 2048, 904] and S.packet_sizes(4096, 2048) == [2048, 2048]
    assert S.packet_sizes(0, 2048) == [] and S.packet_sizes(1, 2048) == [1]
    wave = np.arange(5000)
    assert [len(wave[j:j + 2048]) for j in range(0, len(wave), 2048)] == S.packet_sizes(5000, 2048)


class _Bank:
    """What a session reads of a VoiceBank on the host."""
    names, ref_texts, seconds, samples, frames, speeds, target_rms = ["v"], [REF], [3.0], [72000], [282], [None], 0.1
    mel = torch.zeros(1, 282, 100)
    rms = torch.zeros(1)


class _Vocoder:
    def decode_ragged(self, *a, **k):
        raise AssertionError("not reached on the CPU")


def test_session_first_package_state_and_reset():
    model = P.CFM(transformer=P.DiT(**P.config.F5TTS_TINY, text_num_embeds=257, mel_dim=100))
    text = " ".join([SENT] * 4)
    s = I.open_stream(model, _Vocoder(), (_Bank, "v"), batch_frames=2000, nfe_step=2)
    assert s.stats() == dict(prompt_passes=0, groups_enqueued=0, groups_emitted=0, packets=0)
    first = s.plan(text)
    assert first["chunks"] == [SENT + " " + SENT] * 2 and [list(g) for g in first["groups"]] == [[0], [1]]
    again = s.plan(text)                                       # the same client's second request: one chunk
    assert again["chunks"] == [text] and [list(g) for g in again["groups"]] == [[0]]
    s.reset()                                                  # the client left
    assert s.plan(text)["chunks"] == first["chunks"]
    assert s.plan("")["groups"] == [] and list(s.stream("")) == []
    # durations as synthesize_script plans a chunk: text_numerics on the prompt's samples
    rtext, _, dur = I.text_numerics(72000, REF, SENT + " " + SENT, 1.0, None)
    assert first["texts"][0] == rtext + SENT + " " + SENT and first["durations"][0] == dur and first["ends"][0] == dur
    # batch_frames=None: one chunk per group; an int: the first alone, then group_chunks over the rest
    one = I.open_stream(model, _Vocoder(), (_Bank, "v"), nfe_step=2)
    many = " ".join([SENT] * 40)                               # chunks of 366 bytes: 8 sentences each
    p1 = one.plan(many)
    assert [list(g) for g in p1["groups"]] == [[k] for k in range(len(p1["chunks"]))]
    big = I.open_stream(model, _Vocoder(), (_Bank, "v"), batch_frames=10**6, nfe_step=2)
    p2 = big.plan(many)
    assert p2["chunks"] == p1["chunks"] and [list(g) for g in p2["groups"]] == [[0], list(range(1, len(p2["chunks"])))]
    with pytest.raises(ValueError, match="no voice"):
        I.open_stream(model, _Vocoder(), (_Bank, "w"))
    for bad in (dict(sample_format="u8"), dict(chunk_size=0), dict(lookahead=-1), dict(batch_frames=0)):
        with pytest.raises(ValueError):
            I.open_stream(model, _Vocoder(), (_Bank, "v"), **bad)
    with pytest.raises(_lib.F5Error, match="out_rate"):
        I.open_stream(model, _Vocoder(), (_Bank, "v"), out_rate=4000)
