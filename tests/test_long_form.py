"""CPU: the host side of the batched long-form path (infer.synthesize_long, `batched=True`) -- the integer cross-fade plan
against the host fold it restates, the per-sample fold of include/f5_hip.h against numpy, the chunk grouping, the
f5_wave_crossfade declaration / export / binding, its argument checks (they precede every HIP call, so they need no
device) and the refusals that must come before a device is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

from f5_tts_amd import _lib
from f5_tts_amd import infer as I

F5_EINVAL = -1
NAME = "f5_wave_crossfade"
SR = 24000

# (piece lengths, cross-fade samples): two pieces per sample, pieces shorter than the fade (three and more pieces over one sample,
# a later piece starting before an earlier one), one-sample pieces (n = 1), no fade, a fade longer than a middle piece
LENGTH_SETS = [([256, 256, 512], 100), ([30, 10, 5, 40], 16), ([8, 3, 3, 3, 20], 6), ([1, 1, 1], 4), ([50, 60], 0),
               ([2048, 256, 1024], 3600), ([77], 16)]


def pieces_of(lens, seed=0):
    g = np.random.default_rng(seed)
    return [g.standard_normal(n).astype(np.float32) for n in lens]


def host_fold(pieces, cf):
    """The yardstick: the existing host cross-fade, cast to f32."""
    assert int(cf / SR * SR) == cf, "cf / 24000 does not survive cross_fade_concat's int(duration * 24000)"
    return I.cross_fade_concat(pieces, cf / SR).astype(np.float32)


@pytest.mark.parametrize("lens,cf", LENGTH_SETS)
def test_cross_fade_plan_matches_the_host_fold(lens, cf):
    offs, ns, total = I.cross_fade_plan(lens, cf)
    assert total == len(host_fold(pieces_of(lens), cf))
    assert len(offs) == len(ns) == len(lens) and offs[0] == 0 and ns[0] == 0
    end = lens[0]
    for i in range(1, len(lens)):
        assert ns[i] == (min(cf, end, lens[i]) if cf > 0 else 0)
        assert offs[i] == end - ns[i] and offs[i] >= 0
        end = offs[i] + lens[i]
    assert end == total


@pytest.mark.parametrize("lens,cf", LENGTH_SETS)
def test_per_sample_fold_of_the_header_is_the_host_fold_bit_for_bit(lens, cf):
    """The arithmetic include/f5_hip.h documents for f5_wave_crossfade, evaluated per output sample in float64."""
    pieces = pieces_of(lens, seed=1)
    offs, ns, total = I.cross_fade_plan(lens, cf)
    out = np.empty(total, np.float32)
    for p in range(total):
        v = None
        for i, x in enumerate(pieces):
            j = p - offs[i]
            if not 0 <= j < lens[i]:
                continue
            if i > 0 and j < ns[i]:
                n = ns[i]
                if n == 1:
                    fi, fo = 0.0, 1.0
                elif j == n - 1:
                    fi, fo = 1.0, 0.0
                else:
                    step = 1.0 / (n - 1)
                    fi, fo = j * step + 0.0, j * (-step) + 1.0
                v = v * fo + float(x[j]) * fi
            else:
                v = float(x[j])
        out[p] = np.float32(v)
    assert np.array_equal(out.view(np.int32), host_fold(pieces, cf).view(np.int32))


def test_group_chunks_budget_order_and_max_chunks():
    d = [50, 60, 70, 300, 20, 20, 20, 90]
    runs = I.group_chunks(d, 200)
    assert [list(r) for r in runs] == [[0, 1], [2], [3], [4, 5, 6], [7]]     # 3 * 70 > 200; 300 alone is over the budget
    assert [k for r in runs for k in r] == list(range(len(d)))
    for r in runs:
        assert len(r) == 1 or len(r) * max(d[k] for k in r) <= 200
    assert [list(r) for r in I.group_chunks(d, None)] == [list(range(8))]
    assert [len(r) for r in I.group_chunks([10] * 7, None, max_chunks=3)] == [3, 3, 1]
    assert [len(r) for r in I.group_chunks([10] * 7, 25, max_chunks=3)] == [2, 2, 2, 1]
    assert [len(r) for r in I.group_chunks([10] * 130, None)] == [64, 64, 2]
    assert I.group_chunks([], 100) == []
    assert [list(r) for r in I.group_chunks([500], 100)] == [[0]]


def test_wave_crossfade_is_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "f5_hip.h")).read()
    assert "f5_wave_crossfade <-" in src, "the header's list of replaced reference interfaces lacks the entry"
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", src), f"{NAME} is not declared in include/f5_hip.h"
    assert hasattr(_lib.load(), NAME), f"{NAME} is not exported by libf5hip.so"
    res, args = _lib.SIGNATURES[NAME]
    # (wav, B, wav_stride, lens_host, cross_fade_samples, out, out_cap, out_len_host, stream)
    assert res is C.c_int32 and len(args) == 9
    assert args[2] is C.c_int64 and args[6] is C.c_int64
    assert args[3] == C.POINTER(C.c_int32) and args[7] == C.POINTER(C.c_int64)


def test_argument_checks_need_no_device():
    lib = _lib.load()
    wav, out = C.c_void_p(4096), C.c_void_p(8192)          # never dereferenced: every call below is refused before a launch
    lens = _lib.int_array([10, 20, 15])
    n = C.c_int64(-7)

    def refused(word, *args):
        assert lib.f5_wave_crossfade(*args, C.byref(n), None) == F5_EINVAL
        msg = lib.f5_last_error()
        assert b"f5_wave_crossfade" in msg and word in msg, msg
        assert n.value == -7, "a refused call wrote out_len_host"

    refused(b"B", wav, 0, 20, lens, 4, out, 100)
    refused(b"B", wav, 65, 20, lens, 4, out, 100)
    refused(b"B", wav, -1, 20, lens, 4, out, 100)
    refused(b"wav", None, 3, 20, lens, 4, out, 100)
    refused(b"lens_host", wav, 3, 20, None, 4, out, 100)
    refused(b"out", wav, 3, 20, lens, 4, None, 100)
    refused(b"lens_host[1]", wav, 3, 20, _lib.int_array([10, 0, 15]), 4, out, 100)
    refused(b"lens_host[2]", wav, 3, 20, _lib.int_array([10, 5, -3]), 4, out, 100)
    refused(b"wav_stride", wav, 3, 19, lens, 4, out, 100)
    assert I.cross_fade_plan([10, 20, 15], 4)[2] == 37
    refused(b"out_cap", wav, 3, 20, lens, 4, out, 36)
    refused(b"out_cap", wav, 3, 20, lens, 0, out, 44)      # no fade: 45 samples


def test_batched_with_streaming_is_refused_before_anything_else():
    gen = I.infer_batch_process((None, SR), "ref", ["text"], None, None, batched=True, streaming=True)
    with pytest.raises(ValueError, match="streaming"):
        next(gen)


def test_batched_refusals_need_no_device():
    class Model:
        device = "cpu"
        vocab_char_map = None

    audio = (torch.zeros(1, 2400), SR)
    with pytest.raises(ValueError, match="64"):
        I.synthesize_long(audio, "ref.", ["a"] * 65, Model(), type("V", (), {"decode_ragged": None})())
    with pytest.raises(NotImplementedError, match="decode_ragged"):
        I.synthesize_long(audio, "ref.", ["a"], Model(), object())
    kor = Model()
    kor._tokenizer_type = "kor_jamo"
    with pytest.raises(NotImplementedError, match="text_tokenizer"):
        I.synthesize_long(audio, "ref.", ["a"], kor, type("V", (), {"decode_ragged": None})())
    with pytest.raises(RuntimeError, match="only runs on a GPU"):
        I.wave_crossfade(torch.zeros(2, 8), [8, 5], 3)
    assert list(I.infer_batch_process(audio, "ref.", [], Model(), None, batched=True)) == [(None, SR, None)]
