"""CPU: the prompt preparation stage (f5_mel_prepare_plan / f5_mel_resample_bank / f5_mel_prepare_ragged, MelSpec.prepare_ragged,
the `prompt_on_device` switch of the infer drivers) as far as it goes without a device: the entry points are declared, exported
and bound; every refusal is decided before the first HIP call; the plan agrees with infer.sinc_resample's output shapes; the
factored kernel builder reproduces the kernels sinc_resample used before it was factored out (a restatement of the old body inside
this file); the switch off takes the old route and returns python floats, the switch on calls prepare_ragged exactly once."""
import ctypes as C
import math
import os
import re

import pytest
import torch

from conftest import ROOT

import f5_tts_amd as P
from f5_tts_amd import _lib
from f5_tts_amd import infer as I
from f5_tts_amd import mel as M

F5_EINVAL, F5_ESTATE = -1, -3
TARGET = 24000
HOP, N_MELS = 256, 100
RATES = (8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000)


def geometry(sr, target=TARGET):
    g = math.gcd(sr, target)
    return sr // g, target // g


def lengths(sr):
    orig, _ = geometry(sr)
    return sorted({n for n in (1, 7, orig - 1, orig, orig + 1, 5003) if n >= 1})


def test_prepare_stage_is_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "f5_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _lib.load()
    for name, nargs in (("f5_mel_prepare_plan", 7), ("f5_mel_resample_bank", 6), ("f5_mel_resample_bank_count", 2),
                        ("f5_mel_prepare_ragged", 13)):
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), f"{name} is not declared in include/f5_hip.h"
        assert hasattr(lib, name), f"{name} is not exported by libf5hip.so"
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int32 and len(args) == nargs
    args = _lib.SIGNATURES["f5_mel_prepare_ragged"][1]
    # (m, base, B, start_host, channels_host, n_host, sr_host, target_sr, target_rms, out, out_capacity, rms_out, stream)
    assert args[3] == C.POINTER(C.c_int64) and args[4] == C.POINTER(C.c_int32) and args[8] is C.c_float and args[10] is C.c_int64


def plan(ns, srs, target=TARGET, B=None):
    B = len(ns) if B is None else B
    lens, starts, total = (C.c_int64 * max(len(ns), 1))(), (C.c_int64 * max(len(ns), 1))(), C.c_int64(-1)
    rc = _lib.load().f5_mel_prepare_plan(B, _lib.int_array(ns), _lib.int_array(srs), target, lens, starts, C.byref(total))
    return rc, list(lens)[:len(ns)], list(starts)[:len(ns)], total.value


# ---- the old body of infer.sinc_resample, restated: what the factored builder has to reproduce bit for bit
def old_sinc_resample(waveform, orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99):
    if orig_freq == new_freq:
        return waveform
    g = math.gcd(int(orig_freq), int(new_freq))
    orig, new = int(orig_freq) // g, int(new_freq) // g
    base_freq = min(orig, new) * rolloff
    width = math.ceil(lowpass_filter_width * orig / base_freq)
    idx = torch.arange(-width, width + orig, dtype=torch.float64)[None, None] / orig
    t = torch.arange(0, -new, -1, dtype=torch.float64)[:, None, None] / new + idx
    t = (t * base_freq).clamp_(-lowpass_filter_width, lowpass_filter_width)
    window = torch.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t = t * math.pi
    kernels = torch.where(t == 0, torch.ones_like(t), t.sin() / t) * window * (base_freq / orig)
    kernels = kernels.to(waveform.dtype)
    n = waveform.shape[-1]
    x = torch.nn.functional.pad(waveform.reshape(-1, n), (width, width + orig))
    y = torch.nn.functional.conv1d(x[:, None], kernels, stride=orig)
    y = y.transpose(1, 2).reshape(x.shape[0], -1)[..., : math.ceil(new * n / orig)]
    return y.reshape(*waveform.shape[:-1], -1), kernels, width


@pytest.mark.parametrize("sr", RATES)
def test_plan_lengths_equal_sinc_resample_shapes_and_the_host_helper(sr):
    ns = lengths(sr)
    rc, lens, starts, total = plan(ns, [sr] * len(ns))
    assert rc == 0, _lib.load().f5_last_error()
    g = torch.Generator().manual_seed(sr)
    run = 0
    for n, ln, st in zip(ns, lens, starts):
        want = I.sinc_resample(torch.randn(1, n, generator=g), sr, TARGET).shape[-1]
        assert ln == want == M.resampled_length(n, sr, TARGET), (sr, n)
        run = (run + 3) // 4 * 4
        assert st == run and st % 4 == 0                                  # packed in order, every start on a 16-byte multiple
        run += ln
    assert total == run


def test_plan_of_mixed_rates_hand_computed():
    # 48000 -> 1/2: 5003 -> 2502; 44100 -> 80/147: 148 -> ceil(11840 / 147) = 81; 16000 -> 3/2: 7 -> 11; 24000: 1001 as is
    assert plan([5003, 148, 7, 1001], [48000, 44100, 16000, 24000]) == (0, [2502, 81, 11, 1001], [0, 2504, 2588, 2600], 3601)
    assert plan([1], [48000]) == (0, [1], [0], 1)


@pytest.mark.parametrize("sr", [r for r in RATES if r != TARGET])
def test_factored_kernel_builder_reproduces_the_old_kernels(sr):
    g = torch.Generator().manual_seed(sr + 1)
    orig, new = geometry(sr)
    for dtype in (torch.float32, torch.float64):
        wav = torch.randn(2, 1234, generator=g).to(dtype)
        want, old_kernels, old_width = old_sinc_resample(wav, sr, TARGET)
        kernels, o, nw, width = M.resample_kernel(sr, TARGET)
        assert (o, nw, width) == (orig, new, old_width) and kernels.dtype == torch.float64
        assert torch.equal(kernels.to(dtype), old_kernels)
        assert torch.equal(I.sinc_resample(wav, sr, TARGET), want)
    bank = M._resample_bank_f32(sr, TARGET)
    assert bank.dtype == torch.float32 and bank.shape == (new, 2 * width + orig) and bank.is_contiguous()
    assert torch.equal(bank, old_kernels.to(torch.float32)[:, 0])


def test_standard_rates_have_small_banks_and_24001_does_not():
    for sr in (8000, 11025, 12000, 16000, 22050, 32000, 44100, 48000, 88200, 96000, 176400, 192000):
        k, orig, new, width = M.resample_kernel(sr, TARGET)
        assert new * (2 * width + orig) == k.numel() < 1 << 16, sr
    orig, new = geometry(24001)
    assert new * (2 * math.ceil(6 * orig / (new * 0.99)) + orig) > 1 << 20


def test_plan_refusals():
    lib = _lib.load()

    def refused(rc, *words):
        msg = lib.f5_last_error()
        assert rc == F5_EINVAL, (rc, msg)
        assert b"f5_mel_prepare_plan" in msg and all(w in msg for w in words), msg

    refused(plan([], [], B=0)[0], b"B")
    refused(plan([5] * 3, [48000] * 3, B=65536)[0], b"B")
    refused(plan([5, 0], [48000, 48000])[0], b"item 1", b"n = 0")
    refused(plan([5, 5, 5], [48000, 44100, 0])[0], b"item 2", b"sr = 0")
    refused(plan([5, 5], [48000, 24001])[0], b"item 1", b"24001", b"2^20")
    refused(plan([5], [48000], target=0)[0], b"target_sr")
    lens, starts, total = (C.c_int64 * 1)(), (C.c_int64 * 1)(), C.c_int64()
    one = _lib.int_array([5])
    for args, word in (((None, one, TARGET, lens, starts, C.byref(total)), b"n_host"), ((one, None, TARGET, lens, starts, C.byref(total)), b"sr_host"),
                       ((one, one, TARGET, None, starts, C.byref(total)), b"len_out"), ((one, one, TARGET, lens, None, C.byref(total)), b"start_out"),
                       ((one, one, TARGET, lens, starts, None), b"total_out")):
        refused(lib.f5_mel_prepare_plan(1, *args), word)


@pytest.fixture(scope="module")
def unloaded_handle():
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.f5_mel_create(1024, HOP, N_MELS, C.byref(h)) == 0       # host bookkeeping only: no table, no bank
    return h


def test_prepare_refusals_without_a_device(unloaded_handle):
    """Every refusal is decided before the first HIP call; the pointers are never dereferenced on the way."""
    lib = _lib.load()
    h = unloaded_handle
    buf = (C.c_float * 4)()
    ptr = C.cast(buf, C.c_void_p)
    ns, srs, chans = [5003, 148, 1001], [48000, 44100, 24000], [2, 1, 2]
    total = plan(ns, srs)[3]

    def call(m=h, base=ptr, B=3, starts=(0, 10006, 10154), ch=chans, n=ns, sr=srs, target=TARGET, rms=0.1, out=ptr, cap=total, rms_out=ptr):
        st = None if starts is None else (C.c_int64 * len(starts))(*starts)
        return lib.f5_mel_prepare_ragged(m, base, B, st, _lib.int_array(ch), _lib.int_array(n), _lib.int_array(sr), target, rms, out, cap,
                                         rms_out, None)

    def refused(rc, *words):
        msg = lib.f5_last_error()
        assert rc == F5_EINVAL, (rc, msg)
        assert b"f5_mel_prepare_ragged" in msg and all(w in msg for w in words), msg

    refused(call(m=None), b"m")
    refused(call(base=None), b"base")
    refused(call(starts=None), b"start_host")
    refused(call(ch=None), b"channels_host")
    refused(call(n=None), b"n_host")
    refused(call(sr=None), b"sr_host")
    refused(call(out=None), b"out")
    refused(call(rms_out=None), b"rms_out")
    refused(call(B=0), b"B")
    refused(call(B=-1), b"B")
    refused(call(B=65536), b"B")
    refused(call(ch=[2, 0, 2]), b"item 1", b"channels")
    refused(call(n=[5003, 148, 0]), b"item 2", b"n = 0")
    refused(call(sr=[0, 44100, 24000]), b"item 0", b"sr = 0")
    refused(call(sr=[48000, 24001, 24000]), b"item 1", b"24001")
    refused(call(starts=(0, -4, 10154)), b"item 1", b"start")
    refused(call(rms=0.0), b"target_rms")
    refused(call(rms=-0.1), b"target_rms")
    refused(call(rms=float("nan")), b"target_rms")
    refused(call(target=0), b"target_sr")
    refused(call(cap=total - 1), b"out_capacity", str(total).encode())
    # valid arguments: the only thing missing is the banks (and nothing was uploaded on the way)
    assert call() == F5_ESTATE and b"item 0" in lib.f5_last_error() and b"f5_mel_resample_bank" in lib.f5_last_error()
    count = C.c_int32(-1)
    assert lib.f5_mel_resample_bank_count(h, C.byref(count)) == 0 and count.value == 0


def test_resample_bank_refusals_without_a_device(unloaded_handle):
    lib = _lib.load()
    h = unloaded_handle
    bank = M._resample_bank_f32(48000, TARGET)
    ptr = C.c_void_p(bank.data_ptr())

    def refused(rc, *words):
        msg = lib.f5_last_error()
        assert rc == F5_EINVAL and b"f5_mel_resample_bank" in msg and all(w in msg for w in words), (rc, msg)

    refused(lib.f5_mel_resample_bank(None, 48000, TARGET, ptr, bank.numel(), None), b"m")
    refused(lib.f5_mel_resample_bank(h, 48000, TARGET, None, bank.numel(), None), b"bank_host")
    refused(lib.f5_mel_resample_bank(h, 0, TARGET, ptr, bank.numel(), None), b"sr")
    refused(lib.f5_mel_resample_bank(h, 24001, TARGET, ptr, bank.numel(), None), b"2^20")
    refused(lib.f5_mel_resample_bank(h, TARGET, TARGET, ptr, bank.numel(), None), b"no bank")
    refused(lib.f5_mel_resample_bank(h, 48000, TARGET, ptr, bank.numel() + 1, None), b"numel")
    refused(lib.f5_mel_resample_bank_count(h, None))


def test_prepare_ragged_has_no_cpu_path_and_checks_its_arguments():
    m = P.mel.MelSpec()
    with pytest.raises(RuntimeError, match="only runs on a GPU"):
        m.prepare_ragged([torch.zeros(2, 500), torch.zeros(600)], [44100, 24000], device="cpu")
    with pytest.raises(ValueError):
        m.prepare_ragged([], [])
    with pytest.raises(ValueError):
        m.prepare_ragged([torch.zeros(2, 500)], [44100, 24000])
    with pytest.raises(ValueError):
        m.prepare_ragged([torch.zeros(1, 2, 500)], [44100])


# ---- the prompt_on_device switch of the drivers, with stub model and vocoder objects
class StubMel:
    """The mel front-end in shape only; counts its calls and keeps what it was given.  prepare_ragged answers as the device
    stage would in shape: 1-D waveforms of the resampled lengths and an rms TENSOR."""

    def __init__(self):
        self.prepared, self.ragged, self.plain = [], [], []

    def prepare_ragged(self, audios, rates, target_rms=0.1, device=None):
        self.prepared.append((audios, rates, target_rms))
        return [torch.zeros(M.resampled_length(a.shape[-1], sr, TARGET)) for a, sr in zip(audios, rates)], torch.full((len(audios),), 0.05)

    def forward_ragged(self, wavs, device=None):
        self.ragged.append(wavs)
        frames = [w.shape[-1] // HOP + 1 for w in wavs]
        return torch.zeros(len(wavs), N_MELS, max(frames)), frames

    def __call__(self, wav):
        self.plain.append(wav)
        return torch.zeros(wav.shape[0], N_MELS, wav.shape[-1] // HOP + 1)


def stub_prompts():
    quiet = torch.full((1, 24000), 0.05)
    loud = torch.full((2, 44100), 0.5)
    loud[1, ::2] *= -0.5
    return [(quiet, 24000, "Hello."), (loud, 44100, "안녕")], ["How are you today?", "반갑습니다"]


def test_prompt_batch_switch():
    prompts, gen = stub_prompts()
    off = StubMel()
    pb = I.prompt_batch(prompts, gen, mel_spec=off)
    assert not off.prepared and len(off.ragged) == 1
    assert all(type(r) is float for r in pb["rms"]) and pb["rms"][0] == pytest.approx(0.05)
    assert [tuple(w.shape) for w in off.ragged[0]] == [(1, 24000), (1, 24000)]
    on = StubMel()
    pd = I.prompt_batch(prompts, gen, mel_spec=on, prompt_on_device=True)
    assert len(on.prepared) == 1 and len(on.ragged) == 1
    audios, rates, trms = on.prepared[0]
    assert audios[0] is prompts[0][0] and audios[1] is prompts[1][0] and rates == [24000, 44100] and trms == 0.1   # raw audio, one call
    assert isinstance(pd["rms"], torch.Tensor) and pd["rms"].shape == (2,)
    assert [tuple(w.shape) for w in on.ragged[0]] == [(24000,), (24000,)]                                              # prepare's own views
    for key in ("lens", "durations", "texts"):
        assert pd[key] == pb[key]
    assert pd["cond"].shape == pb["cond"].shape


class StubModel:
    vocab_char_map = None
    device = "cpu"

    def __init__(self):
        self.mel_spec = StubMel()
        self.sampled = []

    def sample(self, cond, text, duration, *, lens=None, **kw):
        self.sampled.append((cond.shape, list(text), duration.tolist()))
        total = int(max(duration.tolist()))
        return torch.zeros(cond.shape[0], total, N_MELS), None


class StubVocoder:
    def __init__(self):
        self.calls = 0

    def decode_ragged(self, mel, ends, starts, gain=None):
        self.calls += 1
        lens = [(e - s) * HOP for e, s in zip(ends, starts)]
        return torch.ones(len(ends), max(lens)), lens


class ForbidHostReads(torch.Tensor):
    """An rms tensor that fails the test when anything asks for its value on the host."""

    @staticmethod
    def wrap(t):
        return t.as_subclass(ForbidHostReads)

    def item(self):
        raise AssertionError(".item() on the device rms")

    def tolist(self):
        raise AssertionError(".tolist() on the device rms")

    def __float__(self):
        raise AssertionError("float() on the device rms")

    def __bool__(self):
        raise AssertionError("a host branch on the device rms")


def test_synthesize_prompts_switch():
    prompts, gen = stub_prompts()
    model, voc = StubModel(), StubVocoder()
    waves, sr, mels = I.synthesize_prompts(model, voc, prompts, gen, nfe_step=2)
    assert not model.mel_spec.prepared and len(model.mel_spec.ragged) == 1 and voc.calls == 1 and sr == TARGET
    # rms 0.05 < 0.1: ones * 0.05 / 0.1; the stereo prompt's mono rms is above target_rms: left alone
    r0 = I.normalise_prompt(prompts[0][0], 24000)[1]
    assert torch.equal(waves[0], torch.ones_like(waves[0]) * r0 / 0.1) and torch.equal(waves[1], torch.ones_like(waves[1]))

    model, voc = StubModel(), StubVocoder()
    prepare = model.mel_spec.prepare_ragged

    def guarded(*a, **k):
        wavs, rms = prepare(*a, **k)
        rms[1] = 0.4
        return wavs, ForbidHostReads.wrap(rms)

    model.mel_spec.prepare_ragged = guarded
    on, sr, mels_on = I.synthesize_prompts(model, voc, prompts, gen, nfe_step=2, prompt_on_device=True)
    assert len(model.mel_spec.prepared) == 1 and len(model.mel_spec.ragged) == 1 and voc.calls == 1
    assert [w.shape for w in on] == [w.shape for w in waves] and [m.shape for m in mels_on] == [m.shape for m in mels]
    r = torch.tensor(0.05)
    assert torch.equal(on[0].as_subclass(torch.Tensor), torch.ones_like(waves[0]) * r / 0.1)   # the host branch's two operations
    assert torch.equal(on[1].as_subclass(torch.Tensor), torch.ones_like(waves[1]))


def test_synthesize_long_switch(monkeypatch):
    audio = torch.full((2, 44100), 0.02)
    chunks = ["How are you today?", "I am fine, thank you very much."]
    monkeypatch.setattr(I, "wave_crossfade", lambda packed, lens, cf: torch.cat([packed[i, :n] for i, n in enumerate(lens)]))

    model, voc = StubModel(), StubVocoder()
    wave, sr, spec = I.synthesize_long((audio, 44100), "Hello.", chunks, model, voc, nfe_step=2)
    assert not model.mel_spec.prepared and len(model.mel_spec.plain) == 1 and tuple(model.mel_spec.plain[0].shape) == (1, 24000)
    host_sampled = model.sampled

    model, voc = StubModel(), StubVocoder()
    prepare = model.mel_spec.prepare_ragged
    model.mel_spec.prepare_ragged = lambda *a, **k: (lambda w, r: (w, ForbidHostReads.wrap(r)))(*prepare(*a, **k))

    def host_route(*a, **k):
        raise AssertionError("normalise_prompt on the prompt_on_device route")

    monkeypatch.setattr(I, "normalise_prompt", host_route)
    on, sr_on, spec_on = I.synthesize_long((audio, 44100), "Hello.", chunks, model, voc, nfe_step=2, prompt_on_device=True)
    assert len(model.mel_spec.prepared) == 1
    audios, rates, _ = model.mel_spec.prepared[0]
    assert len(audios) == 1 and audios[0] is audio and rates == [44100]                      # B = 1, the raw prompt
    assert tuple(model.mel_spec.plain[0].shape) == (1, 24000)
    assert model.sampled == host_sampled                                                      # the same frame arithmetic, from lengths alone
    assert on.shape == wave.shape and spec_on.shape == spec.shape and sr_on == sr
    # the stub's rms is 0.05 on the device route; the host route measured 0.02
    on = on.as_subclass(torch.Tensor)
    assert torch.equal(on, torch.ones_like(on) * torch.tensor(0.05) / 0.1)


def test_infer_process_passes_the_switch_for_batched_only(monkeypatch):
    seen = {}

    def fake_long(*a, **k):
        seen.update(k)
        return torch.zeros(8), TARGET, torch.zeros(N_MELS, 2)

    monkeypatch.setattr(I, "synthesize_long", fake_long)
    audio = torch.full((1, 24000), 0.2)
    I.infer_process((audio, 24000), "Hello.", "How are you today?", StubModel(), StubVocoder(), show_info=None, batched=True, prompt_on_device=True)
    assert seen["prompt_on_device"] is True
    I.infer_process((audio, 24000), "Hello.", "How are you today?", StubModel(), StubVocoder(), show_info=None, batched=True)
    assert seen["prompt_on_device"] is False
    with pytest.raises(ValueError, match="batched=True"):
        I.infer_process((audio, 24000), "Hello.", "How are you today?", StubModel(), StubVocoder(), show_info=None, prompt_on_device=True)
