"""CPU: the ragged Vocos decode is declared, exported and bound; it validates its arguments without a device; the Python
entry points refuse to run off-GPU; and infer.synthesize_batch hands the vocoder the windows sample() actually ran at
(hand-computed cases, a stub model and a stub vocoder that record their arguments)."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import ROOT

import f5_tts_amd as P
from f5_tts_amd import _lib
from f5_tts_amd import infer as I
from f5_tts_amd.cfm import clamp_durations

F5_EINVAL = -1
NAME = "f5_vocos_decode_ragged"


def test_ragged_decode_is_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "f5_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", src), f"{NAME} is not declared in include/f5_hip.h"
    assert hasattr(_lib.load(), NAME), f"{NAME} is not exported by libf5hip.so"
    res, args = _lib.SIGNATURES[NAME]
    # (v, mel, B, stride_b, stride_c, stride_t, starts_host, ends_host, gain_host, wav, wav_stride, stream)
    assert res is C.c_int32 and len(args) == 12
    assert args[3:6] == [C.c_int64] * 3 and args[10] is C.c_int64
    assert args[6] == C.POINTER(C.c_int32) and args[7] == C.POINTER(C.c_int32) and args[8] == C.POINTER(C.c_float)


def test_null_handle_is_refused_without_a_device():
    lib = _lib.load()
    ends = _lib.int_array([4])
    assert lib.f5_vocos_decode_ragged(None, None, 1, 0, 0, 0, None, ends, None, None, 0, None) == F5_EINVAL
    assert b"f5_vocos_decode_ragged" in lib.f5_last_error()


def test_decode_ragged_has_no_cpu_path():
    v = P.Vocos(P.config.VOCOS_TINY).init_synthetic()
    with pytest.raises(RuntimeError, match="only runs on a GPU") as ragged:
        v.decode_ragged(torch.zeros(2, 100, 8), ends=[8, 5], starts=[0, 1])
    with pytest.raises(RuntimeError) as plain:
        v.decode(torch.zeros(2, 100, 8))
    assert str(ragged.value) == str(plain.value)


def test_clamp_durations_hand_computed():
    text = torch.tensor([[3, 4, 5, -1, -1, -1], [1, 1, 1, 1, 1, 1], [2, -1, -1, -1, -1, -1]])
    lens = torch.tensor([4, 2, 9])
    # max(text length, prompt length) + 1 = 5, 7, 10
    assert clamp_durations(text, lens, 8).tolist() == [8, 8, 10]
    assert clamp_durations(text, lens, torch.tensor([3, 20, 12])).tolist() == [5, 20, 12]
    assert clamp_durations(text, lens, torch.tensor([3, 20, 12]), max_duration=11).tolist() == [5, 11, 11]


class StubModel:
    """Records sample()'s arguments and returns a mel of the padded length sample() would."""
    vocab_char_map = None

    def __init__(self):
        self.calls = []

    def sample(self, cond, text, duration, *, lens=None, **kw):
        self.calls.append(dict(cond=cond, text=text, duration=duration, lens=lens, kw=kw))
        n = int(clamp_durations(text, lens, duration, kw.get("max_duration", 65536)).amax())
        self.mel = torch.arange(cond.shape[0] * n * 100, dtype=torch.float32).view(cond.shape[0], n, 100)
        return self.mel, None


class StubVocoder:
    def __init__(self):
        self.calls = []

    def decode_ragged(self, mel, ends, starts=None, gain=None):
        self.calls.append(dict(mel=mel, ends=ends, starts=starts, gain=gain))
        lens = [(e - s - 1) * 256 for s, e in zip(starts, ends)]
        return torch.zeros(len(ends), max(lens)), lens


@pytest.mark.parametrize("duration,kw,ends", [
    (torch.tensor([30, 6, 40]), {}, [30, 13, 40]),            # item 1: 12 text tokens > 5 prompt frames -> 13
    (25, {}, [25, 25, 25]),                                   # an int applies to every item
    (torch.tensor([30, 6, 40]), {"max_duration": 32}, [30, 13, 32]),
])
def test_synthesize_batch_window_arithmetic(duration, kw, ends):
    text = torch.full((3, 12), -1, dtype=torch.long)
    text[0, :7], text[1, :12], text[2, :3] = 1, 2, 3
    lens = [10, 5, 21]
    cond = torch.zeros(3, 21, 100)
    model, voc = StubModel(), StubVocoder()
    wav, wav_lens, mel = I.synthesize_batch(model, voc, cond, text, duration, lens=lens, gain=[1.0, 0.5, 2.0], steps=4, seed=7, **kw)
    (s,), (d,) = model.calls, voc.calls
    assert s["cond"] is cond and s["text"] is text and s["duration"] is duration
    assert s["lens"].tolist() == lens and s["kw"] == dict(steps=4, seed=7, **kw)
    assert d["ends"] == ends and d["starts"] == lens and d["gain"] == [1.0, 0.5, 2.0]
    assert mel is model.mel
    # the vocoder sees sample()'s [B, N, 100] output as the [B, 100, N] view, not a copy
    assert d["mel"].shape == (3, 100, max(ends)) and d["mel"].data_ptr() == mel.data_ptr() and d["mel"].stride() == (max(ends) * 100, 1, 100)
    assert wav_lens == [(e - l - 1) * 256 for e, l in zip(ends, lens)] and wav.shape == (3, max(wav_lens))


def test_synthesize_batch_tokenises_a_list_of_strings_as_sample_does():
    model, voc = StubModel(), StubVocoder()
    I.synthesize_batch(model, voc, torch.zeros(2, 4, 100), ["abcdefg", "hi"], torch.tensor([6, 9]), lens=[4, 3])
    assert model.calls[0]["text"].tolist() == P.utils.list_str_to_tensor(["abcdefg", "hi"]).tolist()
    assert voc.calls[0]["ends"] == [8, 9] and voc.calls[0]["starts"] == [4, 3]   # 7 bytes of text + 1 > 6


def test_synthesize_batch_is_vocos_only():
    bv = P.BigVGAN(P.config.BIGVGAN_TINY)
    with pytest.raises(NotImplementedError):
        I.synthesize_batch(StubModel(), bv, torch.zeros(1, 4, 100), torch.ones(1, 3, dtype=torch.long), 9, lens=[4])
    with pytest.raises(TypeError):
        I.synthesize_batch(StubModel(), StubVocoder(), torch.zeros(1, 4, 100), torch.ones(1, 3, dtype=torch.long), 9, lens=[4],
                           vocoder=StubVocoder())
