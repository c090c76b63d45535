"""CPU: the ragged mel front-end is declared, exported and bound; f5_mel_ragged_plan (pure host arithmetic) lays the items out
so that every frame of an item lies inside that item's own padded signal; f5_mel_forward_ragged refuses bad arguments before it
touches a device; infer.prompt_batch's text / frame arithmetic against hand-computed cases (a stub mel front-end that returns
zeros of the right frame counts); the argument errors of infer.synthesize_prompts."""
import ctypes as C
import os
import random
import re

import pytest
import torch

from conftest import ROOT

import f5_tts_amd as P
from f5_tts_amd import _lib
from f5_tts_amd import infer as I
from f5_tts_amd.batching import prompt_text_and_frames

F5_EINVAL, F5_ESTATE = -1, -3
N_FFT, HOP, N_MELS = 1024, 256, 100
VARIANTS = {"vocos": 512, "bigvgan": 384}   # reflect padding
LENGTH_SETS = {
    "vocos": [(513, 768, 1023, 1024, 1025), (5000, 513, 33111, 16383, 33280)],
    "bigvgan": [(385, 640, 1024), (385, 16500, 33111)],
}


def test_ragged_front_end_is_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "f5_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _lib.load()
    for name, nargs in (("f5_mel_ragged_plan", 7), ("f5_mel_forward_ragged", 11)):
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), f"{name} is not declared in include/f5_hip.h"
        assert hasattr(lib, name), f"{name} is not exported by libf5hip.so"
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int32 and len(args) == nargs
    args = _lib.SIGNATURES["f5_mel_forward_ragged"][1]
    # (m, wav, B, wav_start_host, nw_host, pad, mag_eps, out, out_stride_b, T_out, stream)
    assert args[3] == C.POINTER(C.c_int64) and args[4] == C.POINTER(C.c_int32) and args[6] is C.c_float and args[8] is C.c_int64


def plan(pad, nws, n_fft=N_FFT, hop=HOP):
    B = len(nws)
    rows, frames = (C.c_int32 * (B + 1))(), (C.c_int32 * B)()
    rc = _lib.load().f5_mel_ragged_plan(n_fft, hop, pad, B, _lib.int_array(nws), rows, frames)
    return rc, list(rows), list(frames)


def check_plan(pad, nws):
    rc, rows, frames = plan(pad, nws)
    assert rc == 0, _lib.load().f5_last_error()
    assert rows[0] == 0
    for b, nw in enumerate(nws):
        P_b = nw + 2 * pad
        assert frames[b] == (nw + 2 * pad - N_FFT) // HOP + 1 >= 1          # the rectangular formula
        assert rows[b + 1] > rows[b]
        assert rows[b + 1] - rows[b] == -(-P_b // HOP) >= frames[b]
        # every frame of the item lies inside the item's own padded signal (the last frame reaches furthest) ...
        for t in (0, frames[b] - 1):
            assert (rows[b] + t) * HOP + N_FFT <= rows[b] * HOP + P_b
        # ... and the padded signal ends before the next item starts
        assert rows[b] * HOP + P_b <= rows[b + 1] * HOP


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_plan_of_the_tested_length_sets_and_of_random_ones(variant):
    pad = VARIANTS[variant]
    for nws in LENGTH_SETS[variant]:
        check_plan(pad, nws)
    rng = random.Random(0)
    for _ in range(200):
        check_plan(pad, [rng.randint(pad + 1, 40_000) for _ in range(rng.randint(1, 16))])


def test_plan_hand_computed():
    # vocos: P = nw + 1024; 513 -> P 1537: 3 frames, 7 rows; 768 -> P 1792: 4 frames, 7 rows; 1025 -> P 2049: 5 frames, 9 rows
    assert plan(512, (513, 768, 1025)) == (0, [0, 7, 14, 23], [3, 4, 5])
    # bigvgan: P = nw + 768; 385 -> P 1153: 1 frame, 5 rows
    assert plan(384, (385,)) == (0, [0, 5], [1])


def test_plan_refusals():
    lib = _lib.load()
    assert plan(512, (513, 512))[0] == F5_EINVAL and b"item 1" in lib.f5_last_error()
    assert plan(100, (500,))[0] == F5_EINVAL and b"item 0" in lib.f5_last_error()       # 700 samples < one frame
    assert plan(-1, (5000,))[0] == F5_EINVAL and b"pad" in lib.f5_last_error()
    rows, frames = (C.c_int32 * 2)(), (C.c_int32 * 1)()
    assert lib.f5_mel_ragged_plan(N_FFT, HOP, 512, 0, _lib.int_array([5000]), rows, frames) == F5_EINVAL
    assert lib.f5_mel_ragged_plan(N_FFT, HOP, 512, 1, None, rows, frames) == F5_EINVAL
    assert plan(512, (2_000_000_000,) * 3)[0] == F5_EINVAL and b"2^24" in lib.f5_last_error()


@pytest.fixture(scope="module")
def unloaded_handle():
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.f5_mel_create(N_FFT, HOP, N_MELS, C.byref(h)) == 0      # host bookkeeping only: no table is loaded
    return h


def test_forward_ragged_refusals_without_a_device(unloaded_handle):
    """Every refusal is decided before the first HIP call; the pointers are never dereferenced on the way."""
    lib = _lib.load()
    h = unloaded_handle
    buf = (C.c_float * 4)()
    wav = out = C.cast(buf, C.c_void_p)
    nws = [5000, 513, 7000]                       # T = 20, 3, 28
    T, stride = 28, 28 * N_MELS

    def call(m=h, wav=wav, B=3, starts=(0, 6000, 7000), nw=nws, pad=512, out=out, stride=stride, T_out=T):
        ws = None if starts is None else (C.c_int64 * len(starts))(*starts)
        return lib.f5_mel_forward_ragged(m, wav, B, ws, _lib.int_array(nw), pad, 0.0, out, stride, T_out, None)

    def refused(rc, *words):
        msg = lib.f5_last_error()
        assert rc == F5_EINVAL, (rc, msg)
        assert b"f5_mel" in msg and all(w in msg for w in words), msg

    refused(call(m=None), b"m")
    refused(call(wav=None), b"wav")
    refused(call(starts=None), b"wav_start_host")
    refused(call(nw=None), b"nw_host")
    refused(call(out=None), b"out")
    refused(call(B=0), b"B")
    refused(call(B=-2), b"B")
    refused(call(pad=-1), b"pad")
    refused(call(starts=(0, -1, 7000)), b"item 1", b"wav_start")
    refused(call(nw=[5000, 512, 7000]), b"item 1")                     # nw <= pad
    refused(call(nw=[5000, 2000, 500], pad=100), b"item 2")            # 500 + 200 < n_fft
    refused(call(T_out=27), b"T_out")
    refused(call(stride=stride - 1), b"out_stride_b")
    refused(call(nw=[2_000_000_000] * 3, T_out=1 << 30, stride=1 << 40), b"2^24")
    # valid arguments: the only thing missing is the tables
    assert call() == F5_ESTATE and b"not loaded" in lib.f5_last_error()


def test_forward_ragged_has_no_cpu_path():
    m = P.mel.MelSpec()
    with pytest.raises(RuntimeError, match="only runs on a GPU") as ragged:
        m.forward_ragged([torch.zeros(5000), torch.zeros(1, 6000)], device="cpu")
    with pytest.raises(RuntimeError) as plain:
        m.forward(torch.zeros(1, 5000))
    assert str(ragged.value) == str(plain.value)
    with pytest.raises(ValueError):
        m.forward_ragged([])


class StubMel:
    """forward_ragged of the vocos front-end in shape only: zeros of the right frame counts; keeps what it was given."""

    def forward_ragged(self, wavs):
        self.wavs = wavs
        frames = [w.shape[-1] // HOP + 1 for w in wavs]
        return torch.zeros(len(wavs), N_MELS, max(frames)), frames


def test_prompt_batch_hand_computed():
    quiet = torch.full((1, 24000), 0.05)                                   # rms 0.05 < 0.1: scaled up to 0.1
    loud = torch.full((2, 44100), 0.5)                                     # stereo, 44.1 kHz, rms 0.5: left alone
    loud[1] *= -1.0                                                        # ... and a mono mix of exactly zero would show
    loud[1, ::2] *= -1.0
    short = torch.full((1, 12800), 0.2)
    prompts = [(quiet, 24000, "Hello."), (loud, 44100, "안녕"), (short, 24000, "Good morning!")]
    gen = ["How are you today?", "반갑습니다", "Yes."]
    mel = StubMel()
    pb = I.prompt_batch(prompts, gen, mel_spec=mel)
    # frames: 24000 // 256 + 1 = 94; 44100 samples at 44.1 kHz -> 24000 at 24 kHz -> 94; 12800 // 256 + 1 = 51
    assert pb["lens"] == [94, 94, 51]
    assert pb["cond"].shape == (3, 94, N_MELS)
    # "Hello." ends in a single-byte character: "Hello. " = 7 bytes, 18 bytes to speak: 94 + int(94 / 7 * 18) = 94 + 241
    # "안녕" ends in a three-byte character: 6 bytes, no space, 15 bytes to speak: 94 + int(94 / 6 * 15) = 94 + 235
    # "Good morning! " = 14 bytes, 4 bytes to speak: 51 + int(51 / 14 * 4) = 51 + 14
    assert pb["texts"] == ["Hello. How are you today?", "안녕반갑습니다", "Good morning! Yes."]
    assert pb["durations"] == [335, 329, 65]
    for (audio, sr, rt), gt, n, text, total in zip(prompts, gen, pb["lens"], pb["texts"], pb["durations"]):
        assert (text, total) == prompt_text_and_frames(n, rt, gt, 1.0)
    assert pb["rms"][0] == pytest.approx(0.05) and pb["rms"][2] == pytest.approx(0.2)
    assert pb["rms"][1] == float(torch.sqrt(torch.mean(torch.square(loud.mean(dim=0, keepdim=True)))))
    # what the front-end saw: [1, nw] at 24 kHz, exactly normalise_prompt's / prompt_numerics' audio
    assert [tuple(w.shape) for w in mel.wavs] == [(1, 24000), (1, 24000), (1, 12800)]
    assert torch.equal(mel.wavs[0], quiet * 0.1 / torch.sqrt(torch.mean(torch.square(quiet))))
    assert torch.equal(mel.wavs[2], short)
    for (audio, sr, rt), gt, w, r in zip(prompts, gen, mel.wavs, pb["rms"]):
        a, rms, _, ref_len, _ = I.prompt_numerics(audio, sr, rt, gt)
        assert torch.equal(w, a) and r == rms and ref_len == w.shape[-1] // HOP
        a2, r2 = I.normalise_prompt(audio, sr, 0.1)
        assert torch.equal(a2, a) and r2 == rms


def test_prompt_batch_speed_and_errors():
    p = [(torch.full((1, 24000), 0.2), 24000, "Hello.")]
    assert I.prompt_batch(p, ["How are you today?"], speed=2.0, mel_spec=StubMel())["durations"] == [94 + 120]   # int(94 / 7 * 18 / 2)
    with pytest.raises(ValueError):
        I.prompt_batch(p, ["a", "b"], mel_spec=StubMel())
    with pytest.raises(ValueError):
        I.prompt_batch([], [], mel_spec=StubMel())


class StubModel:
    vocab_char_map = None
    mel_spec = StubMel()
    device = "cpu"


class StubVocoder:
    def decode_ragged(self, *a, **k):
        raise AssertionError("not reached")


def test_synthesize_prompts_argument_errors():
    p = [(torch.full((1, 24000), 0.2), 24000, "Hello.")]
    with pytest.raises(NotImplementedError, match="decode_ragged"):
        I.synthesize_prompts(StubModel(), P.BigVGAN(P.config.BIGVGAN_TINY), p, ["Hi there."])
    with pytest.raises(ValueError):
        I.synthesize_prompts(StubModel(), StubVocoder(), p, ["a", "b"])
    with pytest.raises(ValueError):
        I.synthesize_prompts(StubModel(), StubVocoder(), [], [])
    kor = StubModel()
    kor._tokenizer_type = "kor_jamo"
    with pytest.raises(NotImplementedError, match="text_tokenizer"):
        I.synthesize_prompts(kor, StubVocoder(), p, ["안녕하세요"])
