"""Measures of the engine's own output that need no other model (csrc/dtw.hip; the arithmetic contract is in include/f5_hip.h).

`mel_distance` is DTW-aligned mel-cepstral distortion between pairs of mels, for a ragged batch in one call on the device: orthonormal
DCT-II cepstra 1 .. n_cep of the natural-log mel, the Euclidean frame distance with MCD's constant, the symmetric (1, 2, 1) step
pattern, D(n-1, m-1) / (n + m) in dB.  It is an MFCC-style distance: comparable between checkpoints, precisions and sampler settings
on the same held-out set, NOT comparable to published MCD figures (those use WORLD / SPTK cepstra).  The driver that scores
`sample()`'s free-running output per fine-tune is `infer.heldout_distance`."""
from __future__ import annotations

import ctypes as C
import dataclasses
import math

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


def _plan(entry: str, a_frames, b_frames, n_cep: int) -> tuple[list[int], int]:
    a_frames, b_frames = [int(v) for v in a_frames], [int(v) for v in b_frames]
    if len(a_frames) != len(b_frames):
        raise ValueError(f"{entry[3:]}: {len(a_frames)} lengths of a for {len(b_frames)} of b (need one pair each)")
    P = len(a_frames)
    order, need = (C.c_int32 * max(P, 1))(), C.c_int64()
    _lib.check(getattr(_lib.load(), entry)(P, _lib.int_array(a_frames), _lib.int_array(b_frames), int(n_cep), order, C.byref(need)), entry)
    return list(order)[:P], need.value


def mel_distance_plan(a_frames, b_frames, *, n_cep: int = 13) -> tuple[list[int], int]:
    """f5_mel_distance_plan (pure host arithmetic): (the order in which the workgroups take the pairs -- largest n * m first, ties
    by index --, the bytes of the per-device workspace the call holds: the cepstra and the tables, never an n x m matrix)."""
    return _plan("f5_mel_distance_plan", a_frames, b_frames, n_cep)


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


def _side(entries, who: str, no_gpu: str = _NO_GPU):
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
    items, dev, base, starts = ragged_items(rows, None, no_gpu, f"{who}: the items are on different devices")
    return items, dev, base, starts, int(rows[0].shape[1])


def _pairs(who: str, a, b):
    """Both sides of a call as the library takes them: (keep-alive tensors, device, P, frames of a, frames of b, args) with
    args(lo, hi) the leading arguments of f5_mel_distance / f5_mel_align for pairs [lo, hi)."""
    a, b = list(a), list(b)
    if not a or len(a) != len(b):
        raise ValueError(f"{who}: {len(a)} entries of a for {len(b)} of b (need one pair each, at least one)")
    keep_a, dev, base_a, starts_a, stride_a = _side(a, who)
    keep_b, dev_b, base_b, starts_b, stride_b = _side(b, who)
    if dev != dev_b:
        raise ValueError(f"{who}: a and b are on different devices")
    mels = {int(_rows(e, who).shape[1]) for e in a + b}
    if len(mels) != 1:
        raise ValueError(f"{who}: every entry needs the same number of mel bins (got {sorted(mels)})")
    n_mels = mels.pop()
    frames_a = [int(_rows(e, who).shape[0]) for e in a]
    frames_b = [int(_rows(e, who).shape[0]) for e in b]

    def args(lo, hi):
        i64 = lambda arr: (C.c_int64 * (hi - lo))(*arr[lo:hi])   # noqa: E731
        return (C.c_void_p(base_a), C.c_void_p(base_b), hi - lo, i64(starts_a), _lib.int_array(frames_a[lo:hi]), stride_a, i64(starts_b),
                _lib.int_array(frames_b[lo:hi]), stride_b, n_mels)
    return (keep_a, keep_b), dev, len(a), frames_a, frames_b, args


def mel_distance(a, b, *, n_cep: int = 13) -> torch.Tensor:
    """DTW-aligned mel-cepstral distortion of P pairs in ONE f5_mel_distance (include/f5_hip.h): a and b are equal-length lists,
    every entry an f32 [frames, mel] tensor or a view descriptor (tensor [B, N, mel], item, start, frames) -- item b of `sample()`'s
    output, frames [lens_b, dur_b), is scored where it lies.  Device items of one side with a common row stride are passed by offset;
    otherwise the side is packed once (wave.ragged_items).  1 <= frames <= 4096, 1 <= n_cep <= min(64, mel - 1), mel <= 256.
    Returns f64 [P] on the device, in dB per unit of path weight; nothing is read back and nothing synchronises.  A pair's value does
    not depend on the batch it is scored in, and value(a, b) == value(b, a) bit for bit."""
    keep, dev, P, _, _, args = _pairs("mel_distance", a, b)
    out = torch.empty(P, device=dev, dtype=torch.float64)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().f5_mel_distance(*args(0, P), int(n_cep), _ptr(out), _stream_ptr(dev)), "f5_mel_distance")
    del keep
    return out


# ---------------------------------------------------------------------------------------------------- the alignment and the prosody
MAX_TRACE_BYTES = 1 << 26           # csrc/dtw.hip's kMaxTraceBytes: back-pointers of one f5_mel_align
PROSODY_SUMS = ("diff", "diff2", "x", "y", "xy", "x2", "y2")


def trace_bytes(n: int, m: int) -> int:
    """The bytes of back-pointers f5_mel_align holds for one n x m pair: a 32-bit word per thread and 16 / W rows of the longer side."""
    cols, rows = min(int(n), int(m)), max(int(n), int(m))
    w = strip_width(cols)
    per = DTW_MAX_STRIP // w
    return 4 * (-(-rows // per)) * (-(-cols // w))


def mel_alignment_plan(a_frames, b_frames, *, n_cep: int = 13) -> tuple[list[int], int]:
    """f5_mel_align_plan (pure host arithmetic): mel_distance_plan for mel_alignment -- the same order, and a workspace that also
    holds the back-pointers, 2 bits per cell."""
    return _plan("f5_mel_align_plan", a_frames, b_frames, n_cep)


def mel_alignment(a, b, *, n_cep: int = 13):
    """mel_distance with its path (f5_mel_align; include/f5_hip.h): a and b as mel_distance takes them.  Returns (dist, path,
    path_start, path_len): dist f64 [P], bit for bit mel_distance(a, b); path int32 [sum (n + m - 1), 2] on the device, pair p's
    cells (i, j) -- frame i of a against frame j of b -- in rows path_start[p] .. path_start[p] + path_len[p], in forward order from
    (0, 0) to (n - 1, m - 1); path_start a host list (the cumulative n + m - 1); path_len int32 [P] on the device, 0 for a pair
    whose distance is not finite.  On equal sums the diagonal predecessor wins, then (i - 1, j), then (i, j - 1).  Nothing is read
    back and nothing synchronises.  A batch whose back-pointers exceed MAX_TRACE_BYTES goes down in several calls."""
    keep, dev, P, frames_a, frames_b, args = _pairs("mel_alignment", a, b)
    path_start = [0]
    for n, m in zip(frames_a, frames_b):
        path_start.append(path_start[-1] + max(n + m - 1, 0))
    dist = torch.empty(P, device=dev, dtype=torch.float64)
    path_len = torch.empty(P, device=dev, dtype=torch.int32)
    path = torch.empty(max(path_start[-1], 1), 2, device=dev, dtype=torch.int32)
    # consecutive runs of pairs, each under the cap (a pair over it by itself is the library's to refuse)
    runs, lo, held = [], 0, 0
    for p in range(P):
        need = trace_bytes(frames_a[p], frames_b[p]) if frames_a[p] > 0 and frames_b[p] > 0 else 0
        if p > lo and held + need > MAX_TRACE_BYTES:
            runs.append((lo, p))
            lo, held = p, 0
        held += need
    runs.append((lo, P))
    with torch.cuda.device(dev):
        for lo, hi in runs:
            _lib.check(_lib.load().f5_mel_align(*args(lo, hi), int(n_cep), C.c_void_p(dist.data_ptr() + 8 * lo),
                                                C.c_void_p(path_len.data_ptr() + 4 * lo),
                                                C.c_void_p(path.data_ptr() + 8 * path_start[lo]), _stream_ptr(dev)), "f5_mel_align")
    del keep
    return dist, path, path_start[:P], path_len


def pitch_lags(sample_rate: int, fmin: float, fmax: float) -> tuple[int, int]:
    """(tau_min, tau_max) of a search range in Hz: floor(sample_rate / fmax), ceil(sample_rate / fmin)."""
    return int(math.floor(sample_rate / fmax)), int(math.ceil(sample_rate / fmin))


def pitch_track(waves, lens=None, *, sample_rate: int = 24000, hop: int = 256, first_centre: int = 0, frames=None,
                window: int = 1024, fmin: float = 60.0, fmax: float = 600.0, threshold: float = 0.15):
    """YIN pitch tracks of a ragged batch of mono waveforms in ONE f5_pitch_track (csrc/pitch.hip; the arithmetic contract is in
    include/f5_hip.h).  waves: a list of 1-D f32 tensors, or an f32 [B, L_max] device tensor with `lens` (item i is waves[i, :lens[i]],
    what `decode_ragged` returns), read where they lie; host tensors go down in one copy (wave.ragged_items).  Track frame t is
    centred on sample first_centre + t * hop: MelSpec's frame t of the same wave with first_centre = 0 and the default frames
    len // hop + 1 (vocos), with first_centre = hop // 2 and frames = len // hop (bigvgan).  The lags searched are pitch_lags(sample_rate,
    fmin, fmax): 40 .. 400 at the defaults.  Returns (f0, ap, frames): f64 device tensors packed item after item, frames[i] values
    each -- f0 in Hz, 0 where the frame is unvoiced; ap the normalised difference at the chosen lag (the minimum over the range
    where unvoiced) -- and the host list of frame counts.  Nothing is read back and nothing synchronises.
    These are raw YIN frames: no smoothing over time, no octave correction -- a few frames of subharmonic energy report the octave
    below.  `pitch_track_pyin` is the smoothed tracker (pYIN candidates and a Viterbi decode over them)."""
    waves, ns, frames = _waves_and_frames("pitch_track", waves, lens, hop, frames)
    tau_min, tau_max = pitch_lags(int(sample_rate), float(fmin), float(fmax))
    items, dev, base, starts = ragged_items(waves, None, "pitch_track only runs on a GPU (there is no CPU path)",
                                            "pitch_track: the waveforms are on different devices")
    total = max(sum(max(f, 0) for f in frames), 1)
    f0 = torch.empty(total, device=dev, dtype=torch.float64)
    ap = torch.empty(total, device=dev, dtype=torch.float64)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().f5_pitch_track(C.c_void_p(base), len(ns), starts, _lib.int_array(ns), int(sample_rate), int(hop),
                                              int(first_centre), _lib.int_array(frames), int(window), tau_min, tau_max,
                                              float(threshold), _ptr(f0), _ptr(ap), _stream_ptr(dev)), "f5_pitch_track")
    del items
    return f0, ap, frames


def _waves_and_frames(who: str, waves, lens, hop, frames):
    """pitch_track's reading of its waveforms: (the items as 1-D tensors, their lengths, their frame counts)."""
    if isinstance(waves, torch.Tensor):
        if waves.dim() != 2 or lens is None or len(lens) != waves.shape[0]:
            raise ValueError(f"{who}: a tensor of waves must be [B, L_max] with one length per row (or pass a list of 1-D waveforms)")
        if any(int(n) > waves.shape[1] for n in lens):
            raise ValueError(f"{who}: lens exceed the tensor's {waves.shape[1]} samples")
        waves = [waves[b, :int(n)] for b, n in enumerate(lens)]
    else:
        waves = list(waves)
        if lens is not None:
            waves = [w[:int(n)] for w, n in zip(waves, lens)]
    if not waves or any(w.dim() != 1 for w in waves):
        raise ValueError(f"{who}: need at least one waveform, each 1-D")
    ns = [int(w.shape[0]) for w in waves]
    frames = [n // int(hop) + 1 for n in ns] if frames is None else [int(f) for f in frames]
    if len(frames) != len(ns):
        raise ValueError(f"{who}: {len(frames)} frame counts for {len(ns)} waveforms")
    return waves, ns, frames


# ---------------------------------------------------------------------------------------------------- pYIN
MAX_THRESHOLDS, MAX_BINS, MAX_REACH = 256, 512, 63           # csrc/pitch.hip's kMaxThresholds, kMaxBins, kMaxReach


@dataclasses.dataclass(frozen=True)
class PyinTables:
    """The host tables of the two pYIN stages (include/f5_hip.h), f64 CPU tensors: w [N] the weight of threshold i / N; edge [M + 1]
    the bin edges in Hz, ascending; centre [M]; trans [M, 2 * reach + 1], entry [i, k] the weight of going from bin i to bin
    i + k - reach.  sample_rate, tau_min and tau_max are the search range they were built for."""
    sample_rate: int
    tau_min: int
    tau_max: int
    w: torch.Tensor
    edge: torch.Tensor
    centre: torch.Tensor
    reach: int
    trans: torch.Tensor

    @property
    def n(self) -> int:
        return int(self.w.numel())

    @property
    def bins(self) -> int:
        return int(self.centre.numel())


def _f64(values) -> torch.Tensor:
    return torch.as_tensor(values, dtype=torch.float64).to("cpu").contiguous()


def _f64_ptr(t: torch.Tensor):
    return C.cast(C.c_void_p(t.data_ptr()), C.POINTER(C.c_double))


def pyin_tables(sample_rate: int = 24000, fmin: float = 60.0, fmax: float = 600.0, *, n_thresholds: int = 100, beta=(2, 18),
                bins_per_semitone: int = 5, max_semitones_per_frame: int = 5) -> PyinTables:
    """The tables of pYIN for a search range, built on the host in f64 (the device has no transcendental function to call).
    w_i = F(i / N) - F((i - 1) / N) for the N = n_thresholds thresholds i / N, F the CDF of the Beta prior over YIN's threshold: for
    beta = (2, 18), Mauch and Dixon's prior of mean 0.1, the closed form 1 - (1 - s)^19 - 19 s (1 - s)^18; any other (a, b) through
    scipy.special.betainc.  Bins: M = ceil(12 bins_per_semitone log2(hi / lo)) geometric bins from lo = sample_rate / (tau_max + 1)
    to hi = sample_rate / (tau_min - 1), the range a refined candidate of the lags pitch_lags(sample_rate, fmin, fmax) can reach:
    edge[m] = lo (hi / lo)^(m / M), centre[m] = lo (hi / lo)^((m + 0.5) / M).  Transitions: a triangle of half-width reach =
    bins_per_semitone * max_semitones_per_frame bins (weight reach + 1 - |offset|), each source bin's row divided by its sum over
    the destinations that exist."""
    sample_rate, n = int(sample_rate), int(n_thresholds)
    tau_min, tau_max = pitch_lags(sample_rate, float(fmin), float(fmax))
    reach = int(bins_per_semitone) * int(max_semitones_per_frame)
    if not 1 <= n <= MAX_THRESHOLDS:
        raise ValueError(f"pyin_tables: n_thresholds = {n} (need 1 <= n_thresholds <= {MAX_THRESHOLDS})")
    if tau_min < 2 or tau_min >= tau_max:
        raise ValueError(f"pyin_tables: fmin = {fmin}, fmax = {fmax} give the lags {tau_min} .. {tau_max} (need 2 <= tau_min < tau_max)")
    if not 1 <= reach <= MAX_REACH:
        raise ValueError(f"pyin_tables: a band of {reach} bins per frame (need 1 <= bins_per_semitone * max_semitones_per_frame <= {MAX_REACH})")
    a, b = beta
    if (a, b) == (2, 18):
        def cdf(s):
            return 1.0 - (1.0 - s) ** 19 - 19.0 * s * (1.0 - s) ** 18
    else:
        try:
            from scipy.special import betainc       # the package's one optional dependency: only a non-default prior needs it
        except ImportError as e:
            raise ImportError(f"pyin_tables: beta = {beta!r} needs scipy (scipy.special.betainc); the default (2, 18) does not") from e

        def cdf(s):
            return float(betainc(float(a), float(b), s))
    w = [cdf(i / n) - cdf((i - 1) / n) for i in range(1, n + 1)]
    lo, hi = sample_rate / (tau_max + 1), sample_rate / (tau_min - 1)
    M = int(math.ceil(12 * int(bins_per_semitone) * math.log2(hi / lo)))
    if not 2 <= M <= MAX_BINS:
        raise ValueError(f"pyin_tables: {M} bins from {lo:.1f} to {hi:.1f} Hz (need 2 <= bins <= {MAX_BINS}: fewer bins_per_semitone)")
    edge = [lo * (hi / lo) ** (m / M) for m in range(M + 1)]
    centre = [lo * (hi / lo) ** ((m + 0.5) / M) for m in range(M)]
    trans = []
    for i in range(M):
        row = [float(reach + 1 - abs(k - reach)) if 0 <= i + k - reach < M else 0.0 for k in range(2 * reach + 1)]
        total = math.fsum(row)
        trans.append([v / total for v in row])
    return PyinTables(sample_rate, tau_min, tau_max, _f64(w), _f64(edge), _f64(centre), reach, _f64(trans))


def pyin_bytes(frames_total: int, bins: int) -> int:
    """f5_pitch_decode_bytes: the back-pointers of one f5_pitch_decode, a byte per frame, bin and voicing."""
    return 2 * int(bins) * int(frames_total)


def _tables_for(who: str, tables, sample_rate, fmin, fmax) -> PyinTables:
    """The tables of a call: built for its range where none are given; given ones must be for its sample rate, and for its lag
    range where fmin / fmax are given (None: the tables' own range is taken)."""
    if (fmin is None) != (fmax is None):
        raise ValueError(f"{who}: give both fmin and fmax, or neither")
    if tables is None:
        return pyin_tables(sample_rate, *((60.0, 600.0) if fmin is None else (fmin, fmax)))
    if tables.sample_rate != int(sample_rate):
        raise ValueError(f"{who}: the tables were built for {tables.sample_rate} Hz, the waves are at {int(sample_rate)} Hz")
    if fmin is not None and pitch_lags(int(sample_rate), float(fmin), float(fmax)) != (tables.tau_min, tables.tau_max):
        raise ValueError(f"{who}: the tables were built for the lags {tables.tau_min} .. {tables.tau_max}, fmin = {fmin} and fmax = {fmax} "
                         f"give {pitch_lags(int(sample_rate), float(fmin), float(fmax))} (leave fmin and fmax out to take the tables' range)")
    w = tables.w
    if w.dim() != 1 or not 1 <= w.numel() <= MAX_THRESHOLDS:
        raise ValueError(f"{who}: the tables need 1 <= N <= {MAX_THRESHOLDS} weights in w [N]")
    return tables


def pitch_candidates(waves, lens=None, *, sample_rate: int = 24000, hop: int = 256, first_centre: int = 0, frames=None,
                     window: int = 1024, fmin: float | None = None, fmax: float | None = None, p_absent: float = 0.01,
                     tables: PyinTables | None = None):
    """pYIN's stage 1 for a ragged batch in ONE f5_pitch_candidates (csrc/pitch.hip; the contract is in include/f5_hip.h): every
    threshold i / N of the prior makes YIN's choice on `pitch_track`'s own d', and a frame's candidates are the lags that got votes.
    waves, lens, sample_rate, hop, first_centre, frames, window: pitch_track's.  fmin / fmax: 60 / 600 Hz where both are left out.  tables:
    `pyin_tables(sample_rate, fmin, fmax)` by default; given ones must have been built for sample_rate, and either fmin / fmax are
    left out (the tables bring their lag range) or they name the tables' own lags -- anything else is refused, not ignored.  p_absent: the share of its weight a threshold
    that no lag is under gives to the frame's deepest dip.  Returns (count int32 [F], lag int32 [F, N], f0 f64 [F, N], prob f64
    [F, N], frames) on the device, F frames packed item after item: a frame's count candidates in ascending lag, zeros behind them.
    Nothing is read back and nothing synchronises."""
    who = "pitch_candidates"
    waves, ns, frames = _waves_and_frames(who, waves, lens, hop, frames)
    tab = _tables_for(who, tables, sample_rate, fmin, fmax)
    items, dev, base, starts = ragged_items(waves, None, f"{who} only runs on a GPU (there is no CPU path)",
                                            f"{who}: the waveforms are on different devices")
    total, N = max(sum(max(f, 0) for f in frames), 1), tab.n
    w = _f64(tab.w)                                 # (host, f64, contiguous, whatever a hand-built PyinTables holds)
    count = torch.empty(total, device=dev, dtype=torch.int32)
    lag = torch.empty(total, N, device=dev, dtype=torch.int32)
    f0 = torch.empty(total, N, device=dev, dtype=torch.float64)
    prob = torch.empty(total, N, device=dev, dtype=torch.float64)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().f5_pitch_candidates(C.c_void_p(base), len(ns), starts, _lib.int_array(ns), tab.sample_rate, int(hop),
                                                   int(first_centre), _lib.int_array(frames), int(window), tab.tau_min, tab.tau_max, N,
                                                   _f64_ptr(w), float(p_absent), _ptr(count), _ptr(lag), _ptr(f0), _ptr(prob),
                                                   _stream_ptr(dev)), "f5_pitch_candidates")
    del items
    return count, lag, f0, prob, frames


def pitch_decode(count, f0, prob, frames, tables: PyinTables, *, p_switch: float = 0.01):
    """pYIN's stage 2 in ONE f5_pitch_decode: a Viterbi decode per item over pitch bin x voicing, which picks one candidate per frame
    or "unvoiced"; a move of more than tables.reach bins between two frames is outside the band and is not made.  count int32 [F],
    f0 and prob f64 [F, N] on the device as pitch_candidates returns them (a frame's candidates in array order), frames the host
    list of the items' frame counts.  p_switch: the probability of a change of voicing between two frames.  Returns (f0 f64 [F], 0
    where unvoiced; voiced_prob f64 [F], the frame's summed candidate probability) on the device.  The back-pointers (pyin_bytes)
    are a tensor of this call.  Nothing is read back and nothing synchronises."""
    who = "pitch_decode"
    frames = [int(f) for f in frames]
    total = sum(max(f, 0) for f in frames)
    if count.device.type != "cuda" or f0.device != count.device or prob.device != count.device:
        raise ValueError(f"{who} only runs on a GPU (there is no CPU path): count, f0 and prob must be on one device")
    if f0.dim() != 2 or prob.shape != f0.shape or count.numel() != f0.shape[0] or f0.shape[0] < max(total, 1):
        raise ValueError(f"{who}: need count [F], f0 and prob [F, N] with F >= the {total} frames of the items")
    if count.dtype != torch.int32 or f0.dtype != torch.float64 or prob.dtype != torch.float64:
        raise ValueError(f"{who}: count must be int32, f0 and prob float64")
    dev, N, M = count.device, int(f0.shape[1]), tables.bins
    count, f0, prob = count.contiguous(), f0.contiguous(), prob.contiguous()
    if tables.edge.numel() != M + 1 or tuple(tables.trans.shape) != (M, 2 * tables.reach + 1):
        raise ValueError(f"{who}: the tables need edge [M + 1] and trans [M, 2 * reach + 1] for their {M} bins")
    need = pyin_bytes(max(total, 1), M)
    work = torch.empty(need, device=dev, dtype=torch.uint8)
    out = torch.empty(max(total, 1), device=dev, dtype=torch.float64)
    voiced = torch.empty(max(total, 1), device=dev, dtype=torch.float64)
    edge, centre, trans = _f64(tables.edge), _f64(tables.centre), _f64(tables.trans)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().f5_pitch_decode(_ptr(count), _ptr(f0), _ptr(prob), N, len(frames), _lib.int_array(frames), M,
                                               _f64_ptr(edge), _f64_ptr(centre), int(tables.reach), _f64_ptr(trans), float(p_switch),
                                               _ptr(work), need, _ptr(out), _ptr(voiced), _stream_ptr(dev)), "f5_pitch_decode")
    return out, voiced


def pitch_track_pyin(waves, lens=None, *, sample_rate: int = 24000, hop: int = 256, first_centre: int = 0, frames=None,
                     window: int = 1024, fmin: float | None = None, fmax: float | None = None, p_switch: float = 0.01,
                     p_absent: float = 0.01, tables: PyinTables | None = None):
    """Smoothed pitch tracks of a ragged batch: pYIN (Mauch and Dixon 2014) in two launches, `pitch_candidates` then `pitch_decode`,
    with pitch_track's arguments (without the threshold; fmin / fmax and tables as pitch_candidates reads them), packing and rules: returns (f0, voiced_prob, frames), f64 device tensors
    packed item after item -- f0 in Hz, 0 where the decoded state is unvoiced; voiced_prob the summed probability of the frame's
    candidates -- and the host list of frame counts.  Nothing is read back and nothing synchronises.  An item's track is the same
    alone, in any batch and in any order.  Where YIN reports the octave below for a few frames, the decode keeps the track inside
    the band of `max_semitones_per_frame` per frame.  What it is not: WORLD's F0 (DIO / Harvest), or librosa's pyin (no Boltzmann
    prior over troughs, linear probabilities); digital silence, whose d' is flat, puts its p_absent vote on the smallest lag every
    frame, and such a stretch decodes as voiced at sample_rate / tau_min unless p_absent = 0."""
    who = "pitch_track_pyin"
    tab = _tables_for(who, tables, sample_rate, fmin, fmax)
    count, _, f0, prob, frames = pitch_candidates(waves, lens, sample_rate=sample_rate, hop=hop, first_centre=first_centre, frames=frames,
                                                  window=window, fmin=fmin, fmax=fmax, p_absent=p_absent, tables=tab)
    out, voiced = pitch_decode(count, f0, prob, frames, tab, p_switch=p_switch)
    return out, voiced, frames


def prosody(a_f0, b_f0, path, path_start, path_len):
    """The sums of the classical objective prosody numbers along the alignment, per pair, with plain torch ops on the device in f64
    and without a readback.  a_f0 / b_f0: a list of P f64 tracks per side (Hz, 0 = unvoiced; pair p's have n_p and m_p frames) or
    (packed track, host list of frame counts) as pitch_track returns them; path, path_start, path_len: mel_alignment's.  Returns a
    dict of device tensors [P]: "cells" (path cells), "both_voiced" (cells voiced on both sides), "vuv_mismatch" (voiced on one side
    only), int64; and over the both-voiced cells, with x = log2 f0_a and y = log2 f0_b, the f64 sums "diff" (x - y), "diff2",
    "x", "y", "xy", "x2", "y2" (PROSODY_SUMS).  The counts are exact; the f64 sums are accumulated by index_add_, whose order on the
    device is not fixed, so they can differ in the last bits from run to run."""
    def packed(side):
        if isinstance(side, tuple):
            track, counts = side
            counts = [int(c) for c in counts]
        else:
            counts = [int(t.shape[0]) for t in side]
            track = torch.cat([t.reshape(-1) for t in side])
        off = [0]
        for c in counts:
            off.append(off[-1] + c)
        return track.to(torch.float64), off[:-1]
    dev = path.device
    fa, off_a = packed(a_f0)
    fb, off_b = packed(b_f0)
    P = len(path_start)
    if len(off_a) != P or len(off_b) != P:
        raise ValueError(f"prosody: {len(off_a)} tracks of a and {len(off_b)} of b for {P} paths")
    slots = path.shape[0]
    bounds = torch.tensor(list(path_start)[1:] + [slots], device=dev)
    pair = torch.bucketize(torch.arange(slots, device=dev), bounds, right=True).clamp_(max=P - 1)   # the pair a slot belongs to
    start = torch.tensor(list(path_start), device=dev)[pair]
    live = torch.arange(slots, device=dev) - start < path_len.to(torch.int64)[pair]
    ia = torch.tensor(off_a, device=dev)[pair] + path[:, 0].to(torch.int64)
    ib = torch.tensor(off_b, device=dev)[pair] + path[:, 1].to(torch.int64)
    ia = torch.where(live, ia, torch.zeros_like(ia)).clamp_(0, fa.numel() - 1)       # (dead slots hold scratch)
    ib = torch.where(live, ib, torch.zeros_like(ib)).clamp_(0, fb.numel() - 1)
    va, vb = fa.to(dev)[ia], fb.to(dev)[ib]
    voiced_a, voiced_b = live & (va > 0), live & (vb > 0)
    both = voiced_a & voiced_b
    one = torch.ones((), device=dev, dtype=torch.float64)
    x = torch.log2(torch.where(both, va, one))
    y = torch.log2(torch.where(both, vb, one))

    def total(v, dtype):
        return torch.zeros(P, device=dev, dtype=dtype).index_add_(0, pair, v.to(dtype))
    out = {"cells": total(live, torch.int64), "both_voiced": total(both, torch.int64),
           "vuv_mismatch": total(voiced_a ^ voiced_b, torch.int64)}
    terms = {"diff": x - y, "diff2": (x - y) * (x - y), "x": x, "y": y, "xy": x * y, "x2": x * x, "y2": y * y}
    for name in PROSODY_SUMS:
        out[name] = total(terms[name], torch.float64)
    return out


# ---------------------------------------------------------------------------------------------------- speaker similarity
MOM_CHUNK, MOM_MAX_CEP, MOM_MAX_DIM = 64, 32, 64    # csrc/speaker.hip's kMomChunk, kMaxCep, kMaxDim


@dataclasses.dataclass(frozen=True)
class Moments:
    """Gaussian statistics of S sets of cepstral vectors, on the device (f5_cep_moments; include/f5_hip.h): count int32 [S] (-1: a
    segment with a non-finite frame), mean f64 [S, C], scatter f64 [S, C (C + 1) / 2] -- the centred sums sum (v_p - mean_p)
    (v_q - mean_q), upper triangle packed row-major --, with C = n_cep * (1 + deltas)."""
    count: torch.Tensor
    mean: torch.Tensor
    scatter: torch.Tensor
    n_cep: int
    deltas: bool

    @property
    def dim(self) -> int:
        return int(self.n_cep) * (2 if self.deltas else 1)

    def __len__(self) -> int:
        return int(self.count.shape[0])


def gate_sum_of(gate_db, n_mels: int) -> float:
    """f5_cep_moments' gate_sum for a gate of `gate_db` dB of mean log-mel amplitude below the segment's loudest frame, in double
    on the host: gate_db * ln 10 / 20 * n_mels.  None: -1.0 (no gate)."""
    if gate_db is None:
        return -1.0
    gate_db = float(gate_db)
    if not gate_db >= 0.0:
        raise ValueError(f"cepstral_moments: gate_db = {gate_db} (need gate_db >= 0, or None for no gate)")
    return gate_db * math.log(10.0) / 20.0 * int(n_mels)


def cepstral_moments_plan(frames, *, n_cep: int = 13, deltas: bool = False) -> int:
    """f5_cep_moments_plan (pure host arithmetic): the bytes of the per-device workspace a call over segments of these frame counts
    holds."""
    frames = [int(f) for f in frames]
    need = C.c_int64()
    _lib.check(_lib.load().f5_cep_moments_plan(len(frames), _lib.int_array(frames), int(n_cep), int(bool(deltas)), C.byref(need)),
               "f5_cep_moments_plan")
    return need.value


def cepstral_moments(entries, *, n_cep: int = 13, deltas: bool = False, select=None, gate_db=None) -> Moments:
    """Count, mean and centred scatter of the cepstral vectors of S sets of mel frames in ONE f5_cep_moments (include/f5_hip.h):
    entries as mel_distance takes a side -- f32 [frames, mel] tensors or view descriptors (tensor [B, N, mel], item, start, frames),
    read where they lie.  The vectors are mel_distance's cepstra 1 .. n_cep (n_cep <= 32) and, with deltas, their regression deltas
    over +-2 frames of the segment.  select: an optional bool / uint8 tensor with one entry per frame of the call, entry after entry
    (a caller with pitch tracks can pass f0 > 0); gate_db: keep the frames whose mean log-mel amplitude is within gate_db dB of
    the entry's loudest frame (None, the default: every frame -- there is no recommended threshold).  Returns Moments on the
    device; nothing is read back, and with device entries and a device mask (or none) nothing synchronises -- a host mask, like
    host entries, goes down in one pageable copy, which does.  An entry's record does not depend on the batch it is in."""
    who = "cepstral_moments"
    entries = list(entries)
    if not entries:
        raise ValueError(f"{who}: need at least one entry")
    if not 1 <= int(n_cep) <= MOM_MAX_CEP:          # (before anything is allocated from it)
        raise ValueError(f"{who}: n_cep = {n_cep} (need 1 <= n_cep <= min({MOM_MAX_CEP}, mel - 1))")
    rows = [_rows(e, who) for e in entries]
    keep, dev, base, starts, stride = _side(rows, who, f"{who} only runs on a GPU (there is no CPU path)")
    mels = {int(t.shape[1]) for t in rows}
    if len(mels) != 1:
        raise ValueError(f"{who}: every entry needs the same number of mel bins (got {sorted(mels)})")
    n_mels = mels.pop()
    frames = [int(t.shape[0]) for t in rows]
    S, dim = len(frames), int(n_cep) * (2 if deltas else 1)
    mask = None
    if select is not None:
        mask = torch.as_tensor(select).reshape(-1)
        if mask.numel() != sum(frames):
            raise ValueError(f"{who}: select has {mask.numel()} entries for the {sum(frames)} frames of the call")
        mask = (mask != 0).to(device=dev, dtype=torch.uint8).contiguous()
    count = torch.empty(S, device=dev, dtype=torch.int32)
    mean = torch.empty(S, dim, device=dev, dtype=torch.float64)
    scatter = torch.empty(S, dim * (dim + 1) // 2, device=dev, dtype=torch.float64)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().f5_cep_moments(C.c_void_p(base), S, starts, _lib.int_array(frames), stride, n_mels, int(n_cep),
                                              int(bool(deltas)), _ptr(mask), gate_sum_of(gate_db, n_mels), _ptr(count), _ptr(mean),
                                              _ptr(scatter), _stream_ptr(dev)), "f5_cep_moments")
    del keep
    return Moments(count, mean, scatter, int(n_cep), bool(deltas))


def _triu(dim: int, device):
    idx = torch.triu_indices(dim, dim, device=device)          # row-major over the upper triangle: the records' packing
    return idx[0], idx[1]


def merge_moments(moments: Moments, groups):
    """Pools records by label: groups[s] is record s's label (any hashable).  Returns (Moments with one record per label, the labels
    in order of first appearance).  A label's records are folded in item order with the pairwise update n = n_a + n_b, d = mean_b -
    mean_a, mean = mean_a + d n_b / n, scatter = scatter_a + scatter_b + d d^T n_a n_b / n, in torch f64 ops on the device, without
    a readback: what the moments of the concatenated frames would be, up to rounding.  A record with count 0 adds nothing; one with
    count -1 makes its label's record count -1 and NaN.  The index table goes down in one (pageable, hence synchronous) copy; the
    fold is then a dozen small torch launches per round, all labels at once, and the number of rounds is the largest number of
    records under one label: it runs once per evaluation, not per batch, and is the part to restructure if one label ever holds
    thousands of records."""
    groups = list(groups)
    S, dim = len(moments), moments.dim
    if len(groups) != S:
        raise ValueError(f"merge_moments: {len(groups)} labels for {S} records")
    labels, members = [], {}
    for s, g in enumerate(groups):
        if g not in members:
            members[g] = []
            labels.append(g)
        members[g].append(s)
    dev = moments.count.device
    U = len(labels)
    rounds = max(len(m) for m in members.values())
    # round r takes every label's r-th record, all labels at once; the whole index table goes down in ONE copy (-1: no such record)
    table = torch.tensor([[members[g][r] if r < len(members[g]) else -1 for g in labels] for r in range(rounds)]).to(dev)
    p, q = _triu(dim, dev)
    n = torch.zeros(U, device=dev, dtype=torch.float64)
    bad = torch.zeros(U, device=dev, dtype=torch.bool)
    mean = torch.zeros(U, dim, device=dev, dtype=torch.float64)
    scatter = torch.zeros(U, dim * (dim + 1) // 2, device=dev, dtype=torch.float64)
    zero = torch.zeros((), device=dev, dtype=torch.float64)
    for r in range(rounds):
        src = table[r].clamp(min=0)
        cb = torch.where(table[r] >= 0, moments.count[src], torch.zeros_like(moments.count[src]))
        bad |= cb < 0
        live = (cb > 0).unsqueeze(1)
        nb = cb.clamp(min=0).to(torch.float64)
        tot = n + nb
        safe = torch.where(tot > 0, tot, torch.ones_like(tot))
        d = torch.where(live, moments.mean[src] - mean, zero)          # (no record, an empty or a bad one: d = 0 and no scatter)
        scatter = scatter + torch.where(live, moments.scatter[src], zero) + d[:, p] * d[:, q] * (n * nb / safe).unsqueeze(1)
        mean = mean + d * (nb / safe).unsqueeze(1)
        n = tot
    nan = torch.full((), float("nan"), device=dev, dtype=torch.float64)
    count = torch.where(bad, torch.full_like(n, -1.0), n).to(torch.int32)
    mean = torch.where(bad.unsqueeze(1), nan, mean)
    scatter = torch.where(bad.unsqueeze(1), nan, scatter)
    return Moments(count, mean, scatter, moments.n_cep, moments.deltas), labels


def gaussian_divergence(a: Moments, b: Moments, pairs=None):
    """The raw terms of the second-order divergence between record i of a and record j of b for every (i, j) in `pairs` (None:
    record s of a against record s of b) in ONE f5_gauss_divergence (include/f5_hip.h).  Returns (terms f64 [P, 4] = (tr_ij, tr_ji,
    q_i, q_j), status int32 [P]) on the device: tr_ij = trace(cov_i^-1 cov_j), q_i = (mean_i - mean_j)^T cov_i^-1 (mean_i - mean_j).
    A pair with a side of count <= C, or whose covariance is not positive definite in f64, gets NaNs and status 1.  Nothing is read
    back and nothing synchronises; `speaker_numbers` turns the terms into numbers after the readback."""
    who = "gaussian_divergence"
    if a.dim != b.dim:
        raise ValueError(f"{who}: a has {a.dim}-dimensional records, b {b.dim}")
    if a.count.device.type != "cuda" or b.count.device != a.count.device:
        raise RuntimeError(f"{who} only runs on a GPU (there is no CPU path): both sets of records must be on one device")
    if pairs is None:
        if len(a) != len(b):
            raise ValueError(f"{who}: {len(a)} records of a for {len(b)} of b (give pairs)")
        pairs = [(s, s) for s in range(len(a))]
    pairs = [(int(i), int(j)) for i, j in pairs]
    if not pairs:
        raise ValueError(f"{who}: need at least one pair")
    dev, P = a.count.device, len(pairs)
    sides = [(m.count.contiguous(), m.mean.contiguous(), m.scatter.contiguous()) for m in (a, b)]
    terms = torch.empty(P, 4, device=dev, dtype=torch.float64)
    status = torch.empty(P, device=dev, dtype=torch.int32)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().f5_gauss_divergence(*[_ptr(t) for t in sides[0]], len(a), *[_ptr(t) for t in sides[1]], len(b), a.dim, P,
                                                   _lib.int_array([i for i, _ in pairs]), _lib.int_array([j for _, j in pairs]),
                                                   _ptr(terms), _ptr(status), _stream_ptr(dev)), "f5_gauss_divergence")
    del sides
    return terms, status


def speaker_numbers(terms, C: int) -> dict:
    """The two numbers of a pair from gaussian_divergence's terms (host arithmetic after the readback): terms a sequence of four
    values (tr_ij, tr_ji, q_i, q_j), or of P such rows -- then lists come back.  "kl": the symmetric Kullback-Leibler divergence
    between the two Gaussians in nats, 0.5 ((tr_ij + tr_ji) - 2 C) + 0.5 (q_i + q_j) (the log-determinants cancel).  "sphericity":
    log(tr_ij tr_ji / C^2), the arithmetic-harmonic sphericity measure -- covariances alone, so a constant offset of the cepstral
    mean (a channel) does not move it.  NaN terms (a singular pair) give NaN.  Neither is SIM or an embedding cosine."""
    rows = terms.tolist() if hasattr(terms, "tolist") else list(terms)
    single = not rows or not isinstance(rows[0], (list, tuple))
    kl, sph = [], []
    for tr_ij, tr_ji, q_i, q_j in ([rows] if single else rows):
        kl.append(0.5 * ((tr_ij + tr_ji) - 2 * C) + 0.5 * (q_i + q_j))
        ratio = tr_ij * tr_ji / (C * C)
        sph.append(math.log(ratio) if ratio > 0 else float("nan"))
    return dict(kl=kl[0], sphericity=sph[0]) if single else dict(kl=kl, sphericity=sph)
