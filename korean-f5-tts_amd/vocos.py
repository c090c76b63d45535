"""Vocos vocoder with the surface the reference's harness uses: `vocoder.decode(mel[B, 100, T]) -> wav[B, T']`
(infer/utils_infer.py:114-137,702-703; eval/eval_infer_batch.py:206), plus `decode_ragged` for a batch of windows of unequal
length in one pass.  Arithmetic runs in libf5hip (csrc/vocos.hip).
Parameter names are those of charactr/vocos-mel-24khz's `pytorch_model.bin` (backbone.* / head.*)."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from . import weights as W
from ._lib import _ptr, _stream_ptr
from .config import VOCOS_24K
from .native import NativeVocoder


def idft_basis(n_fft: int) -> tuple[torch.Tensor, torch.Tensor]:
    """(hann window [n_fft], Basis [n_fft, K2]) such that frames = [Re S | Im S | 0-pad] @ Basis^T equals
    irfft(S, n_fft) * hann  (what torch.istft computes per frame).  float64 on the host, rounded once to f32."""
    Fb = n_fft // 2 + 1
    K2 = (2 * Fb + 31) // 32 * 32  # whole 128-byte K-tiles of the f32 LDS-DMA GEMM
    j = torch.arange(n_fft, dtype=torch.float64)[:, None]
    f = torch.arange(Fb, dtype=torch.float64)[None, :]
    ang = 2 * torch.pi * f * j / n_fft
    c = torch.full((1, Fb), 2.0, dtype=torch.float64)
    c[0, 0] = 1.0
    c[0, -1] = 1.0
    win = torch.hann_window(n_fft, dtype=torch.float64)
    re = (c * torch.cos(ang)) * win[:, None] / n_fft
    im = (-c * torch.sin(ang)) * win[:, None] / n_fft
    im[:, 0] = 0.0   # c2r transforms ignore the imaginary part of the DC and Nyquist bins
    im[:, -1] = 0.0
    B = torch.zeros(n_fft, K2, dtype=torch.float64)
    B[:, :Fb] = re
    B[:, Fb:2 * Fb] = im
    return torch.hann_window(n_fft, dtype=torch.float32), B.to(torch.float32)


class Vocos(NativeVocoder):
    _prefix, _load = "f5_vocos", "f5_vocos_load_weight"

    def __init__(self, cfg: dict = VOCOS_24K, device=None):
        super().__init__(cfg)
        if device is not None:
            self.to(device)

    def param_shapes(self):
        return W.vocos_param_shapes(self.cfg)

    def load_state_dict(self, sd, strict=True, assign=False):
        return self._set_state({k: v for k, v in sd.items() if not k.startswith("feature_extractor.")}, strict, "vocos")

    def _create(self, lib, h):
        c = self.cfg
        cfg = _lib.f5_vocos_config()
        cfg.input_channels, cfg.dim, cfg.intermediate_dim = c["input_channels"], c["dim"], c["intermediate_dim"]
        cfg.num_layers, cfg.n_fft, cfg.hop_length = c["num_layers"], c["n_fft"], c["hop_length"]
        return lib.f5_vocos_create(C.byref(cfg), C.byref(h))

    def _aux_tables(self):
        return zip(("aux.hann", "aux.idft_basis"), idft_basis(self.cfg["n_fft"]))

    @torch.no_grad()
    def decode(self, mel: torch.Tensor) -> torch.Tensor:
        """mel f32[B, C, T] -> wav f32[B, (T - 1) * hop]."""
        h = self._handle()
        dev = self._anchor.device
        if mel.device != dev or mel.dtype != torch.float32:
            mel = mel.detach().to(device=dev, dtype=torch.float32)
        B, Cc, T = mel.shape
        assert Cc == self.cfg["input_channels"]
        wav = torch.empty(B, (T - 1) * self.cfg["hop_length"], device=dev, dtype=torch.float32)
        sb, sc, st = mel.stride()   # any view: the callers pass sample()'s [B, T, C] output as .permute(0, 2, 1)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().f5_vocos_decode_strided(h, _ptr(mel), B, T, sb, sc, st, _ptr(wav), _stream_ptr(dev)),
                       "f5_vocos_decode")
        return wav

    @torch.no_grad()
    def decode_ragged(self, mel: torch.Tensor, ends, starts=None, gain=None) -> tuple[torch.Tensor, list[int]]:
        """A ragged batch in one pass (f5_vocos_decode_ragged): item b is frames [starts[b], ends[b]) of row b of mel f32[B, C, T]
        (any view, e.g. sample()'s output as .permute(0, 2, 1) with starts = the prompt lengths and ends = the durations).
        Returns (wav f32[B, L_max], wav_lens): wav[b, :wav_lens[b]] is bit-identical to decode() of that slice alone
        (times gain[b] where gains are given), zeros behind it; wav_lens[b] = (ends[b] - starts[b] - 1) * hop.
        ends / starts: lists or CPU tensors of ints; starts=None: every item starts at frame 0."""
        h = self._handle()
        dev = self._anchor.device
        if mel.device != dev or mel.dtype != torch.float32:
            mel = mel.detach().to(device=dev, dtype=torch.float32)
        B, Cc, T = mel.shape
        assert Cc == self.cfg["input_channels"]
        ends = [int(e) for e in (ends.tolist() if torch.is_tensor(ends) else ends)]
        starts = None if starts is None else [int(s) for s in (starts.tolist() if torch.is_tensor(starts) else starts)]
        gain = None if gain is None else [float(g) for g in (gain.tolist() if torch.is_tensor(gain) else gain)]
        if len(ends) != B or (starts is not None and len(starts) != B) or (gain is not None and len(gain) != B):
            raise ValueError(f"decode_ragged: ends / starts / gain must have one entry per batch row ({B})")
        for b, e in enumerate(ends):
            s0 = starts[b] if starts else 0
            if s0 < 0 or e > T or e - s0 < 2:
                raise ValueError(f"decode_ragged: item {b} is frames [{s0}, {e}) of {T}: need 0 <= start, end <= T and at least 2 frames")
        hop = self.cfg["hop_length"]
        wav_lens = [(e - (starts[b] if starts else 0) - 1) * hop for b, e in enumerate(ends)]
        wav = torch.empty(B, max(wav_lens), device=dev, dtype=torch.float32)
        sb, sc, st = mel.stride()
        with torch.cuda.device(dev):
            _lib.check(_lib.load().f5_vocos_decode_ragged(
                h, _ptr(mel), B, sb, sc, st, _lib.int_array(starts), _lib.int_array(ends),
                None if gain is None else _lib.float_array(gain), _ptr(wav), wav.shape[1], _stream_ptr(dev)),
                "f5_vocos_decode_ragged")
        return wav, wav_lens

    def forward(self, mel):
        return self.decode(mel)
