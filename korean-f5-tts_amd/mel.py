"""Prompt mel front-end with the reference's `MelSpec` surface (model/modules.py:107-146).  mel_spec_type="vocos":
torchaudio MelSpectrogram(n_fft=1024, win=1024, hop=256, n_mels=100, power=1, center=True, norm=None) then
clamp(min=1e-5).log() (modules.py:78-104); mel_spec_type="bigvgan": reflect pad (n_fft - hop) / 2, stft(center=False),
sqrt(re^2 + im^2 + 1e-9), librosa's slaney mel basis, log(clamp(., 1e-5)) (modules.py:33-75).  The arithmetic runs in libf5hip (csrc/mel.hip: strided-view STFT GEMM, magnitude, mel GEMM
with a log epilogue); this file only builds the constant tables on the host.  `forward_ragged` is the reference's
per-prompt loop + `padded_mel_batch` (eval/utils_eval.py:109-148, 17-25) as one pass over the packed rows of every prompt;
`prepare_ragged` is what the drivers do to each prompt in front of it (mono mix, RMS, the gain up to target_rms, torchaudio's
Resample to the model's rate; utils_infer.py:523-533) as one pass on the device (csrc/prompt.hip), from the windowed-sinc bank
that `resample_kernel` builds here on the host.

torchaudio is not installed in the build container, so its HTK filterbank (`melscale_fbanks`, norm=None) is restated
here from its published definition, and so is librosa's slaney filterbank (`librosa.filters.mel`, htk=False,
norm="slaney") for the bigvgan variant -- PARITY UNPINNED for those two tables (no fixture of them exists in the reference)."""
from __future__ import annotations

import ctypes as C
import functools
import math

import torch

from . import _lib
from ._lib import _ptr, _stream_ptr
from .edit import MAX_ITEMS, edit_mask, segment_table
from .native import NativeModule
from .wave import ragged_items


def htk_mel_filterbank(n_freqs: int, n_mels: int, sample_rate: int, f_min: float = 0.0, f_max: float | None = None):
    """torchaudio.functional.melscale_fbanks(n_freqs, f_min, f_max, n_mels, sample_rate, norm=None, mel_scale="htk")
    transposed to [n_mels, n_freqs]."""
    f_max = float(sample_rate // 2) if f_max is None else f_max
    all_freqs = torch.linspace(0, sample_rate // 2, n_freqs)
    m_min = 2595.0 * math.log10(1.0 + f_min / 700.0)
    m_max = 2595.0 * math.log10(1.0 + f_max / 700.0)
    m_pts = torch.linspace(m_min, m_max, n_mels + 2)
    f_pts = 700.0 * (10 ** (m_pts / 2595.0) - 1.0)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts.unsqueeze(0) - all_freqs.unsqueeze(1)          # [n_freqs, n_mels + 2]
    down = (-1.0 * slopes[:, :-2]) / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    fb = torch.clamp(torch.min(down, up), min=0.0)                # [n_freqs, n_mels]
    return fb.t().contiguous()


def slaney_mel_filterbank(n_freqs: int, n_mels: int, sample_rate: int, f_min: float = 0.0, f_max: float | None = None):
    """librosa.filters.mel(sr, n_fft, n_mels, fmin, fmax) with its defaults (slaney scale: linear below 1 kHz, log above;
    area-normalised triangles) -> [n_mels, n_freqs]."""
    f_max = sample_rate / 2.0 if f_max is None else f_max
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, math.log(6.4) / 27.0

    def hz_to_mel(f):
        return min_log_mel + math.log(f / min_log_hz) / logstep if f >= min_log_hz else f / f_sp

    m = torch.linspace(hz_to_mel(f_min), hz_to_mel(f_max), n_mels + 2, dtype=torch.float64)
    mel_f = torch.where(m >= min_log_mel, min_log_hz * torch.exp(logstep * (m - min_log_mel)), f_sp * m)
    fftfreqs = torch.linspace(0, sample_rate / 2.0, n_freqs, dtype=torch.float64)
    fdiff = mel_f[1:] - mel_f[:-1]
    ramps = mel_f[:, None] - fftfreqs[None, :]
    w = torch.clamp(torch.minimum(-ramps[:-2] / fdiff[:-1, None], ramps[2:] / fdiff[1:, None]), min=0.0)
    return (w * (2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels]))[:, None]).to(torch.float32)


def stft_basis(n_fft: int) -> torch.Tensor:
    """[round_up(2F, 4), n_fft]: rows hann[j] cos(2 pi f j / n) (f < F) then hann[j] sin(2 pi f j / n); float64 -> f32."""
    Fb = n_fft // 2 + 1
    ns = (2 * Fb + 3) // 4 * 4
    j = torch.arange(n_fft, dtype=torch.float64)[None, :]
    f = torch.arange(Fb, dtype=torch.float64)[:, None]
    ang = 2 * torch.pi * f * j / n_fft
    win = torch.hann_window(n_fft, dtype=torch.float64)[None, :]
    B = torch.zeros(ns, n_fft, dtype=torch.float64)
    B[:Fb] = torch.cos(ang) * win
    B[Fb:2 * Fb] = torch.sin(ang) * win
    return B.to(torch.float32)


def resample_kernel(orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99):
    """The polyphase windowed-sinc kernel of torchaudio.transforms.Resample(orig_freq, new_freq) with its defaults
    (functional._get_sinc_resample_kernel, resampling_method="sinc_interp_hann"), restated from its published algorithm: returns
    (kernels float64 [new, 1, 2 width + orig], orig, new, width) with orig, new the rates over their gcd.  infer.sinc_resample
    convolves with its cast to the waveform's dtype; the device path (MelSpec.prepare_ragged) uploads its f32 cast."""
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
    return kernels, orig, new, width


@functools.lru_cache(maxsize=32)
def _resample_bank_f32(sr: int, target: int) -> torch.Tensor:
    """f32 [new, 2 width + orig]: what f5_mel_resample_bank takes (computed once per rate pair and process)."""
    return resample_kernel(sr, target)[0][:, 0].to(torch.float32).contiguous()


def resampled_length(n: int, sr: int, target_sample_rate: int = 24_000) -> int:
    """Samples a prompt of n samples at sr Hz has at the target rate, ceil(new * n / orig) in integers: the length of
    infer.sinc_resample's result and of MelSpec.prepare_ragged's item, without a device read."""
    g = math.gcd(int(sr), int(target_sample_rate))
    orig, new = int(sr) // g, int(target_sample_rate) // g
    return -(-new * int(n) // orig)


class MelSpec(NativeModule):
    _prefix, _load, _finalize = "f5_mel", "f5_mel_load", False
    _no_cpu = "the HIP mel front-end only runs on a GPU (there is no CPU path)"

    def __init__(self, n_fft=1024, hop_length=256, win_length=1024, n_mel_channels=100, target_sample_rate=24_000,
                 mel_spec_type="vocos"):
        super().__init__()
        assert mel_spec_type in ["vocos", "bigvgan"]
        if win_length != n_fft:
            raise NotImplementedError("win_length != n_fft is unused by every shipped config")
        self.n_fft, self.hop_length, self.win_length = n_fft, hop_length, win_length
        self.n_mel_channels, self.target_sample_rate = n_mel_channels, target_sample_rate
        self.mel_spec_type = mel_spec_type

    def _create(self, lib, h):
        return lib.f5_mel_create(self.n_fft, self.hop_length, self.n_mel_channels, C.byref(h))

    def _tensors(self):
        Fb = self.n_fft // 2 + 1
        fb = torch.zeros(self.n_mel_channels, (Fb + 31) // 32 * 32)
        make_fb = htk_mel_filterbank if self.mel_spec_type == "vocos" else slaney_mel_filterbank
        fb[:, :Fb] = make_fb(Fb, self.n_mel_channels, self.target_sample_rate)
        return [("aux.dft_basis", stft_basis(self.n_fft)), ("aux.mel_fb", fb)]

    @torch.no_grad()
    def forward(self, wav: torch.Tensor) -> torch.Tensor:
        """wav f32[b, nw] (or [b, 1, nw]) on a GPU -> log-mel f32[b, n_mels, T] (the reference's layout)."""
        if wav.dim() == 3:
            wav = wav.squeeze(1)
        dev = wav.device
        h = self._handle(dev)
        wav = wav.to(torch.float32).contiguous()
        B, nw = wav.shape
        pad, eps = self._variant()
        T = (nw + 2 * pad - self.n_fft) // self.hop_length + 1
        out = torch.empty(B, T, self.n_mel_channels, device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().f5_mel_forward_ex(h, _ptr(wav), B, nw, pad, eps, _ptr(out), _stream_ptr(dev)), "f5_mel_forward")
        return out.permute(0, 2, 1)

    def _variant(self):
        """(reflect padding, magnitude epsilon) of the mel_spec_type."""
        return (self.n_fft // 2, 0.0) if self.mel_spec_type == "vocos" else ((self.n_fft - self.hop_length) // 2, 1e-9)

    @torch.no_grad()
    def forward_ragged(self, wavs, device=None):
        """Prompts of unequal length in one pass (f5_mel_forward_ragged): wavs is a list of f32 [nw_i] (or [1, nw_i]) tensors, on
        the host or on a GPU -> (log-mel f32[B, n_mels, T_max], frames).  mel[i, :, :frames[i]] is bit for bit
        `forward(wavs[i][None])[0]`, the columns behind it are +0.0 (`padded_mel_batch`); like `forward`, the return is a permuted
        view of [B, T_max, n_mels].  Host tensors go down in ONE concatenated copy; device tensors are read where they are.
        device: where host tensors go (default: the device tensors' device, else the current GPU)."""
        wavs = [w.squeeze(0) if w.dim() == 2 and w.shape[0] == 1 else w for w in wavs]
        if not wavs:
            raise ValueError("forward_ragged: no waveform")
        if any(w.dim() != 1 for w in wavs):
            raise ValueError("forward_ragged: every waveform must be [nw] or [1, nw]")
        nws = [int(w.shape[0]) for w in wavs]
        wavs, dev, base, starts = ragged_items(wavs, device, self._no_cpu, "forward_ragged: the waveforms are on different devices")
        lib = _lib.load()
        B = len(wavs)
        pad, eps = self._variant()
        nw_arr = _lib.int_array(nws)
        rows, frames = (C.c_int32 * (B + 1))(), (C.c_int32 * B)()
        _lib.check(lib.f5_mel_ragged_plan(self.n_fft, self.hop_length, pad, B, nw_arr, rows, frames), "f5_mel_ragged_plan")
        frames = list(frames)
        T = max(frames)
        out = torch.empty(B, T, self.n_mel_channels, device=dev, dtype=torch.float32)
        h = self._handle(dev)
        with torch.cuda.device(dev):
            _lib.check(lib.f5_mel_forward_ragged(h, C.c_void_p(base), B, starts, nw_arr, pad, eps, _ptr(out),
                                                 T * self.n_mel_channels, T, _stream_ptr(dev)), "f5_mel_forward_ragged")
        return out.permute(0, 2, 1), frames

    @torch.no_grad()
    def prepare_ragged(self, audios, rates, target_rms=0.1, device=None):
        """What the drivers do to every prompt before its mel -- mono mix, RMS, the gain up to target_rms where the RMS is below it,
        resampling to `target_sample_rate` (infer.normalise_prompt per item) -- in one pass on the device (f5_mel_prepare_ragged;
        the arithmetic contract is in include/f5_hip.h).  audios: a list of f32 [C_i, n_i] (or [n_i]) tensors, on the host or on a
        GPU; rates: their sample rates.  Returns (wavs, rms): wavs[i] is a 1-D view of resampled_length(n_i, rates[i]) samples
        into one packed device buffer, which forward_ragged reads in place; rms is a device f32[B] tensor (the RMS of each mono
        input) that nothing here reads back.  Host tensors go down in ONE concatenated copy; device tensors are read where they
        are (non-contiguous ones are made contiguous first).  A rate whose filter bank would exceed 2^20 elements (e.g. 24001 Hz)
        is refused: resample that prompt on the host (infer.sinc_resample)."""
        audios = [a[None] if a.dim() == 1 else a for a in audios]
        rates = [int(r) for r in rates]
        if not audios:
            raise ValueError("prepare_ragged: no audio")
        if len(rates) != len(audios):
            raise ValueError(f"prepare_ragged: {len(audios)} audios for {len(rates)} rates (need one rate per audio)")
        if any(a.dim() != 2 for a in audios):
            raise ValueError("prepare_ragged: every audio must be [channels, n] or [n]")
        shapes = [(int(a.shape[0]), int(a.shape[1])) for a in audios]
        audios, dev, base, starts = ragged_items(audios, device, self._no_cpu, "prepare_ragged: the audios are on different devices")
        lib = _lib.load()
        B = len(audios)
        n_arr, sr_arr = _lib.int_array([n for _, n in shapes]), _lib.int_array(rates)
        lens, offs, total = (C.c_int64 * B)(), (C.c_int64 * B)(), C.c_int64()
        _lib.check(lib.f5_mel_prepare_plan(B, n_arr, sr_arr, self.target_sample_rate, lens, offs, C.byref(total)), "f5_mel_prepare_plan")
        h = self._handle(dev)
        out = torch.empty(total.value, device=dev, dtype=torch.float32)
        rms = torch.empty(B, device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            self._resample_banks(lib, h, dev, rates)
            _lib.check(lib.f5_mel_prepare_ragged(h, C.c_void_p(base), B, starts, _lib.int_array([c for c, _ in shapes]),
                                                 n_arr, sr_arr, self.target_sample_rate, float(target_rms), _ptr(out), total.value,
                                                 _ptr(rms), _stream_ptr(dev)), "f5_mel_prepare_ragged")
        return [out[o:o + n] for o, n in zip(offs, lens)], rms

    @torch.no_grad()
    def edit_assemble(self, mel, frames, plans):
        """The conditioning of speech editing for a batch in one launch (f5_edit_assemble; the reference's torch.cat chain per
        recording, infer/speech_edit.py:157-195).  mel: the original log-mels f32 [B, n_mels, T_max] as `forward_ragged` (or
        `forward`) returns them -- the permuted view, whose storage [B, T_max, n_mels] is read in place; any other layout is copied
        first; frames: T_i per item; plans: edit.edit_plan's return per item.  Returns (cond f32 [B, D_max, n_mels] -- KEEP frames
        are bit copies of their source frames, EDIT frames and the frames behind D_i are +0.0 --, edit_mask bool [B, D_max] on
        the host (True = keep; built there because CFM.sample reads it there), [D_i])."""
        plans = list(plans)
        frames = [int(t) for t in frames]
        if mel.device.type != "cuda":
            raise RuntimeError(self._no_cpu)
        if mel.dim() != 3 or mel.shape[1] != self.n_mel_channels:
            raise ValueError(f"edit_assemble: mel must be [B, {self.n_mel_channels}, T]")
        B, row, T_max = mel.shape
        if not 1 <= B <= MAX_ITEMS:
            raise ValueError(f"edit_assemble: {B} recordings; one call takes 1 to {MAX_ITEMS}")
        if len(frames) != B or len(plans) != B:
            raise ValueError(f"edit_assemble: {len(frames)} frame counts and {len(plans)} plans for {B} recordings")
        if any(t > T_max for t in frames):
            raise ValueError(f"edit_assemble: frames {frames} exceed the mel's {T_max} columns")
        rows = mel.permute(0, 2, 1)                                            # [B, T_max, n_mels]
        if rows.dtype != torch.float32 or rows.stride(2) != 1 or rows.stride(1) != row or (B > 1 and rows.stride(0) < T_max * row):
            rows = rows.to(torch.float32).contiguous()
        D = [int(d) for _, d in plans]
        counts, flat = segment_table(plans)
        cond = torch.empty(B, max(D), row, device=mel.device, dtype=torch.float32)
        with torch.cuda.device(mel.device):
            _lib.check(_lib.load().f5_edit_assemble(_ptr(rows), B, rows.stride(0) if B > 1 else T_max * row, row, _lib.int_array(frames),
                                                    counts, flat, _lib.int_array(D), _ptr(cond),
                                                    max(D), _stream_ptr(mel.device)), "f5_edit_assemble")
        return cond, edit_mask(plans), D

    def _resample_banks(self, lib, h, dev, rates):
        """Hands the handle the bank of every rate it has not seen (once per rate pair and handle; the handle keeps them)."""
        known = h.__dict__.setdefault("_banks", set())
        for sr in sorted(set(rates) - known - {self.target_sample_rate}):
            bank = _resample_bank_f32(sr, self.target_sample_rate)
            _lib.check(lib.f5_mel_resample_bank(h, sr, self.target_sample_rate, C.c_void_p(bank.data_ptr()), bank.numel(), _stream_ptr(dev)),
                       "f5_mel_resample_bank")
            known.add(sr)
