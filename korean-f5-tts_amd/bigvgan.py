"""BigVGAN v2 vocoder with the surface the reference's harness uses for `mel_spec_type="bigvgan"`:
`vocoder(mel[B, 100, T]) -> wav[B, 1, 256 T]` (infer/utils_infer.py:138-152,705; eval/eval_infer_batch.py:208), plus
`forward_ragged` for a batch of windows of unequal length in one pass and `ragged()`, the view the batch drivers of infer.py take.
Arithmetic runs in libf5hip (csrc/bigvgan.hip).  The reference loads `nvidia/bigvgan_v2_24khz_100band_256x` through an
un-vendored submodule: parameter names are those of that published generator after `remove_weight_norm()`; the
architecture is restated from it (parity unpinned; the checker of tests/test_bigvgan.py is a CPU restatement of the same published design)."""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib
from . import weights as W
from ._lib import _ptr, _stream_ptr
from .config import BIGVGAN_V2_24K
from .native import NativeVocoder


def kaiser_sinc_filter1d(cutoff: float, half_width: float, kernel_size: int) -> torch.Tensor:
    """The low-pass prototype of BigVGAN's alias-free activation (alias_free_activation/torch/filter.py), float32 [k]."""
    even = kernel_size % 2 == 0
    half_size = kernel_size // 2
    A = 2.285 * (half_size - 1) * math.pi * (4 * half_width) + 7.95
    beta = 0.1102 * (A - 8.7) if A > 50.0 else (0.5842 * (A - 21) ** 0.4 + 0.07886 * (A - 21.0) if A >= 21.0 else 0.0)
    window = torch.kaiser_window(kernel_size, beta=beta, periodic=False)
    time = (torch.arange(-half_size, half_size) + 0.5) if even else (torch.arange(kernel_size) - half_size)
    filt = 2 * cutoff * window * torch.sinc(2 * cutoff * time)
    return (filt / filt.sum()).to(torch.float32)


class BigVGAN(NativeVocoder):
    _prefix, _load = "f5_bigvgan", "f5_bigvgan_load_weight"

    def __init__(self, cfg: dict = BIGVGAN_V2_24K, device=None, precision: str = "f32"):
        """precision: "f32" (f32 MFMA throughout) or "f16x3" (the wide stages' convolutions as split-f16 products, include/f5_hip.h
        F5_PREC_F16X3: f32-level results, ~2.5x the f32 GEMM rate)."""
        super().__init__(cfg)
        if precision not in ("f32", "f16x3"):
            raise ValueError("BigVGAN precision must be 'f32' or 'f16x3'")
        self.precision = precision
        self.total_up = 1
        for u in self.cfg["upsample_rates"]:
            self.total_up *= u
        if device is not None:
            self.to(device)

    def param_shapes(self):
        return W.bigvgan_param_shapes(self.cfg)

    def remove_weight_norm(self):
        """The reference calls this after loading (utils_infer.py:151); checkpoints given to load_state_dict are expected
        with plain `weight` tensors (weight_g / weight_v pairs are folded here when present)."""
        return self

    def load_state_dict(self, sd, strict=True, assign=False):
        sd = dict(sd)
        for k in [k for k in sd if k.endswith(".weight_g")]:      # fold torch weight_norm parametrisations: w = g * v / ||v||
            base = k[: -len(".weight_g")]
            g, v = sd.pop(k), sd.pop(base + ".weight_v")
            sd[base + ".weight"] = v * (g / v.flatten(1).norm(dim=1).view(-1, *([1] * (v.dim() - 1))))
        sd = {k: v for k, v in sd.items() if not k.endswith((".filter", ".lowpass.filter"))}   # filter buffers are recomputed
        return self._set_state(sd, strict, "bigvgan")

    def _create(self, lib, h):
        return lib.f5_bigvgan_create(C.byref(self._config()), C.byref(h))

    def _aux_tables(self):
        f = kaiser_sinc_filter1d(0.25, 0.3, 12)     # Activation1d(up_ratio=2, down_ratio=2, kernel 12): cutoff 0.5/2, half width 0.6/2
        return [("aux.up_filter", f), ("aux.down_filter", f)]

    @torch.no_grad()
    def forward(self, mel: torch.Tensor) -> torch.Tensor:
        """mel f32[B, num_mels, T] (any view) -> wav f32[B, 1, T * 256]."""
        h = self._handle()
        dev = self._anchor.device
        if mel.device != dev or mel.dtype != torch.float32:
            mel = mel.detach().to(device=dev, dtype=torch.float32)
        B, Cc, T = mel.shape
        assert Cc == self.cfg["num_mels"]
        wav = torch.empty(B, 1, T * self.total_up, device=dev, dtype=torch.float32)
        sb, sc, st = mel.stride()
        with torch.cuda.device(dev):
            _lib.check(_lib.load().f5_bigvgan_forward(h, _ptr(mel), B, T, sb, sc, st, _ptr(wav), _stream_ptr(dev)),
                       "f5_bigvgan_forward")
        return wav

    def _config(self):
        """The f5_bigvgan_config of this generator (what _create hands to the library)."""
        c = self.cfg
        cfg = _lib.f5_bigvgan_config()
        cfg.num_mels, cfg.upsample_initial_channel = c["num_mels"], c["upsample_initial_channel"]
        cfg.num_upsamples = len(c["upsample_rates"])
        for i, (u, k) in enumerate(zip(c["upsample_rates"], c["upsample_kernel_sizes"])):
            cfg.upsample_rates[i], cfg.upsample_kernel_sizes[i] = u, k
        cfg.num_kernels = len(c["resblock_kernel_sizes"])
        for j, k in enumerate(c["resblock_kernel_sizes"]):
            cfg.resblock_kernel_sizes[j] = k
        cfg.num_dilations = len(c["resblock_dilation_sizes"])
        for m, d in enumerate(c["resblock_dilation_sizes"]):
            cfg.resblock_dilations[m] = d
        cfg.use_tanh_at_final, cfg.use_bias_at_final = int(bool(c.get("use_tanh_at_final"))), int(bool(c.get("use_bias_at_final")))
        cfg.precision = _lib.PRECISIONS[self.precision]
        return cfg

    def ragged_plan(self, frames) -> tuple[list[int], int]:
        """The packed time axis of one ragged call (f5_bigvgan_ragged_plan, host arithmetic): (row_start, gap) -- item b of
        frames[b] frames starts at frame row_start[b], row_start[B] is the packed frame count, and at least `gap` dead frames
        separate consecutive items."""
        frames = [int(f) for f in frames]
        rs, gap = (C.c_int32 * (len(frames) + 1))(), C.c_int32()
        _lib.check(_lib.load().f5_bigvgan_ragged_plan(C.byref(self._config()), len(frames), _lib.int_array(frames), rs, C.byref(gap)),
                   "f5_bigvgan_ragged_plan")
        return list(rs), gap.value

    def _ragged_groups(self, frames, max_frames):
        """Consecutive groups of items, each of at most max_frames packed frames (an item longer than that is a group of its own)."""
        if max_frames is None:
            return [range(len(frames))]
        if int(max_frames) < 1:
            raise ValueError(f"forward_ragged: max_frames = {max_frames}; need at least 1 (or None: one group)")
        groups, i0 = [], 0
        while i0 < len(frames):
            rs, _gap = self.ragged_plan(frames[i0:])
            n = 1
            while i0 + n < len(frames) and rs[n] + frames[i0 + n] <= max_frames:
                n += 1
            groups.append(range(i0, i0 + n))
            i0 += n
        return groups

    @torch.no_grad()
    def forward_ragged(self, mel: torch.Tensor, ends, starts=None, gain=None, max_frames=None) -> tuple[torch.Tensor, list[int]]:
        """A ragged batch in one pass (f5_bigvgan_forward_ragged): item b is frames [starts[b], ends[b]) of row b of mel f32[B, C, T]
        (any view, e.g. sample()'s output as .permute(0, 2, 1) with starts = the prompt lengths and ends = the durations).
        Returns (wav f32[B, L_max], wav_lens): wav[b, :wav_lens[b]] is bit-identical to forward() of that slice alone (times
        gain[b] where gains are given), zeros behind it; wav_lens[b] = (ends[b] - starts[b]) * total_up.
        ends / starts: lists or CPU tensors of ints; starts=None: every item starts at frame 0.
        max_frames: None = one library call for the whole batch; else consecutive groups of items of at most that many packed
        frames (ragged_plan), one call each, which bounds the workspace -- the same bits either way."""
        if mel.dim() != 3 or mel.shape[1] != self.cfg["num_mels"]:
            raise ValueError(f"forward_ragged: mel must be [B, {self.cfg['num_mels']}, T] (got {tuple(mel.shape)})")
        B, _Cc, T = mel.shape
        ends = [int(e) for e in (ends.tolist() if torch.is_tensor(ends) else ends)]
        starts = None if starts is None else [int(s) for s in (starts.tolist() if torch.is_tensor(starts) else starts)]
        gain = None if gain is None else [float(g) for g in (gain.tolist() if torch.is_tensor(gain) else gain)]
        if len(ends) != B or (starts is not None and len(starts) != B) or (gain is not None and len(gain) != B):
            raise ValueError(f"forward_ragged: ends / starts / gain must have one entry per batch row ({B})")
        if B < 1:
            raise ValueError("forward_ragged: need at least one item")
        for b, e in enumerate(ends):
            s0 = starts[b] if starts else 0
            if s0 < 0 or e > T or e - s0 < 1:
                raise ValueError(f"forward_ragged: item {b} is frames [{s0}, {e}) of {T}: need 0 <= start, end <= T and at least 1 frame")
        frames = [e - (starts[b] if starts else 0) for b, e in enumerate(ends)]
        groups = self._ragged_groups(frames, max_frames)
        h = self._handle()
        dev = self._anchor.device
        if mel.device != dev or mel.dtype != torch.float32:
            mel = mel.detach().to(device=dev, dtype=torch.float32)
        wav_lens = [f * self.total_up for f in frames]
        wav = torch.empty(B, max(wav_lens), device=dev, dtype=torch.float32)
        sb, sc, st = mel.stride()
        with torch.cuda.device(dev):
            for g in groups:
                i0, i1 = g.start, g.stop
                _lib.check(_lib.load().f5_bigvgan_forward_ragged(
                    h, _ptr(mel[i0:i1]), i1 - i0, sb, sc, st, None if starts is None else _lib.int_array(starts[i0:i1]),
                    _lib.int_array(ends[i0:i1]), None if gain is None else _lib.float_array(gain[i0:i1]), _ptr(wav[i0:i1]),
                    wav.shape[1], _stream_ptr(dev)), "f5_bigvgan_forward_ragged")
        return wav, wav_lens

    def ragged(self) -> "RaggedBigVGAN":
        """The view to hand to the batch drivers (infer.synthesize_batch / synthesize_long / synthesize_prompts): the same
        handle and weights, with `decode_ragged` = forward_ragged."""
        return RaggedBigVGAN(self)


class RaggedBigVGAN:
    """A thin view of one BigVGAN for the drivers that decode through `vocoder.decode_ragged`: decode_ragged is the vocoder's
    forward_ragged, calling it (or .forward) is the vocoder's own forward; everything else is looked up on the vocoder."""

    def __init__(self, vocoder: BigVGAN):
        self.vocoder = vocoder

    def decode_ragged(self, mel, ends, starts=None, gain=None, max_frames=None):
        return self.vocoder.forward_ragged(mel, ends, starts=starts, gain=gain, max_frames=max_frames)

    def forward(self, mel):
        return self.vocoder.forward(mel)

    def __call__(self, mel):
        return self.vocoder(mel)

    def __getattr__(self, name):
        return getattr(self.vocoder, name)
