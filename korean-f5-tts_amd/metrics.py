"""Measures of the engine's own output that need no other model (csrc/dtw.hip; the arithmetic contract is in include/f5_hip.h).

`mel_distance` is DTW-aligned mel-cepstral distortion between pairs of mels, for a ragged batch in one call on the device: orthonormal
DCT-II cepstra 1 .. n_cep of the natural-log mel, the Euclidean frame distance with MCD's constant, the symmetric (1, 2, 1) step
pattern, D(n-1, m-1) / (n + m) in dB.  It is an MFCC-style distance: comparable between checkpoints, precisions and sampler settings
on the same held-out set, NOT comparable to published MCD figures (those use WORLD / SPTK cepstra).  The driver that scores
`sample()`'s free-running output per fine-tune is `infer.heldout_distance`."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._lib import _ptr, _stream_ptr
from .wave import ragged_items

# csrc/dtw.hip's constants of the same names (kDtwThreads, kDtwMaxStrip, kDtwRowBlock): a pair's shorter side is its column side,
# thread t of the pair's workgroup owns columns [t W, t W + W), W = strip_width(columns); the longer side streams through LDS in
# blocks of DTW_ROW_BLOCK rows.
DTW_THREADS, DTW_MAX_STRIP, DTW_ROW_BLOCK = 256, 16, 32
MAX_FRAMES, MAX_PAIRS, MAX_CEP = DTW_THREADS * DTW_MAX_STRIP, 65535, 64
_NO_GPU = "mel_distance only runs on a GPU (there is no CPU path)"


def strip_width(columns: int) -> int:
    """The strip of a pair whose shorter side has `columns` frames: the smallest power of two W with W * DTW_THREADS >= columns."""
    w = 1
    while w * DTW_THREADS < columns:
        w *= 2
    return w


def mel_distance_plan(a_frames, b_frames, *, n_cep: int = 13) -> tuple[list[int], int]:
    """f5_mel_distance_plan (pure host arithmetic): (the order in which the workgroups take the pairs -- largest n * m first, ties
    by index --, the bytes of the per-device workspace the call holds: the cepstra and the tables, never an n x m matrix)."""
    a_frames, b_frames = [int(v) for v in a_frames], [int(v) for v in b_frames]
    if len(a_frames) != len(b_frames):
        raise ValueError(f"mel_distance_plan: {len(a_frames)} lengths of a for {len(b_frames)} of b (need one pair each)")
    P = len(a_frames)
    order, need = (C.c_int32 * max(P, 1))(), C.c_int64()
    _lib.check(_lib.load().f5_mel_distance_plan(P, _lib.int_array(a_frames), _lib.int_array(b_frames), int(n_cep), order,
                                                C.byref(need)), "f5_mel_distance_plan")
    return list(order)[:P], need.value


def _rows(entry, who: str) -> torch.Tensor:
    """An entry as a [frames, mel] view: a tensor as it is, (tensor [B, N, mel], item, start, frames) as that item's frames."""
    if isinstance(entry, torch.Tensor):
        t = entry
    else:
        t, item, start, frames = entry
        item, start, frames = int(item), int(start), int(frames)
        if t.dim() != 3 or not 0 <= item < t.shape[0] or start < 0 or frames < 0 or start + frames > t.shape[1]:
            raise ValueError(f"{who}: a view must be (tensor [B, N, mel], item, start, frames) inside the tensor")
        t = t[item, start:start + frames]
    if t.dim() != 2:
        raise ValueError(f"{who}: every entry must be [frames, mel] (or a view descriptor)")
    return t


def _side(entries, who: str):
    """One side's items as (keep-alive tensors, device, base pointer, ctypes element offsets, row stride).  Items that lie on the
    device as f32 with unit element stride and one common row stride are passed by offset from the lowest address, where they are;
    anything else is packed once by `ragged_items`' rule (host tensors down in one copy, contiguous f32)."""
    rows = [_rows(e, who) for e in entries]
    in_place = all(t.device.type == "cuda" and t.dtype == torch.float32 and t.stride(1) == 1 for t in rows)
    strides = {int(t.stride(0)) for t in rows if t.shape[0] > 1}
    if in_place and len(strides) <= 1 and len({t.device for t in rows}) == 1:
        stride = strides.pop() if strides else int(rows[0].shape[1])
        if stride >= rows[0].shape[1]:
            base = min(t.data_ptr() for t in rows)
            return rows, rows[0].device, base, (C.c_int64 * len(rows))(*[(t.data_ptr() - base) // 4 for t in rows]), stride
    items, dev, base, starts = ragged_items(rows, None, _NO_GPU, f"{who}: the items are on different devices")
    return items, dev, base, starts, int(rows[0].shape[1])


def mel_distance(a, b, *, n_cep: int = 13) -> torch.Tensor:
    """DTW-aligned mel-cepstral distortion of P pairs in ONE f5_mel_distance (include/f5_hip.h): a and b are equal-length lists,
    every entry an f32 [frames, mel] tensor or a view descriptor (tensor [B, N, mel], item, start, frames) -- item b of `sample()`'s
    output, frames [lens_b, dur_b), is scored where it lies.  Device items of one side with a common row stride are passed by offset;
    otherwise the side is packed once (wave.ragged_items).  1 <= frames <= 4096, 1 <= n_cep <= min(64, mel - 1), mel <= 256.
    Returns f64 [P] on the device, in dB per unit of path weight; nothing is read back and nothing synchronises.  A pair's value does
    not depend on the batch it is scored in, and value(a, b) == value(b, a) bit for bit."""
    a, b = list(a), list(b)
    if not a or len(a) != len(b):
        raise ValueError(f"mel_distance: {len(a)} entries of a for {len(b)} of b (need one pair each, at least one)")
    keep_a, dev, base_a, starts_a, stride_a = _side(a, "mel_distance")
    keep_b, dev_b, base_b, starts_b, stride_b = _side(b, "mel_distance")
    if dev != dev_b:
        raise ValueError("mel_distance: a and b are on different devices")
    mels = {int(_rows(e, "mel_distance").shape[1]) for e in a + b}
    if len(mels) != 1:
        raise ValueError(f"mel_distance: every entry needs the same number of mel bins (got {sorted(mels)})")
    n_mels, P = mels.pop(), len(a)
    frames_a = [int(_rows(e, "mel_distance").shape[0]) for e in a]
    frames_b = [int(_rows(e, "mel_distance").shape[0]) for e in b]
    out = torch.empty(P, device=dev, dtype=torch.float64)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().f5_mel_distance(C.c_void_p(base_a), C.c_void_p(base_b), P, starts_a, _lib.int_array(frames_a), stride_a,
                                               starts_b, _lib.int_array(frames_b), stride_b, n_mels, int(n_cep), _ptr(out),
                                               _stream_ptr(dev)), "f5_mel_distance")
    del keep_a, keep_b
    return out
