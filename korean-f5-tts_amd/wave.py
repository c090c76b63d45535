"""The device waveform calls around sample() as Python functions (csrc/wave.hip, csrc/deliver.hip, csrc/emit.hip, csrc/edit.hip,
csrc/silence.hip): the cross-fade of decoded chunks, the join of a multi-voice script's pieces, the delivery at a client's rate, join
and delivery for many streams in one launch, the splice of the original recording around edited spans, the silence flags and the gather of the clipped signal --
and the two pieces of plumbing every ragged call of the audio side shares: `ragged_items` (a list of host or device tensors as
device items under one base pointer) and `flat_segments` (segment tables as the C entry points read them).  The drivers that call
these are in infer.py, which re-exports them."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._lib import _ptr, _stream_ptr
from .config import HOP_LENGTH
from .edit import segment_table


def ragged_items(tensors, device, no_gpu: str, mixed: str):
    """A list of tensors as the items of one ragged call: picks the device (`device`, else the device tensors' device, else the
    current GPU), sends the host tensors down in ONE concatenated copy (each comes back as a flat 1-D piece of it) and leaves device
    tensors where they are, as contiguous f32.  Returns (items, device, base, starts): one base pointer and a ctypes int64 array of
    element offsets from it -- every f32 tensor is 4-byte aligned.  The caller checks shapes and hands over its own texts: no_gpu for
    the RuntimeError when there is no GPU to run on, mixed for the ValueError when device tensors are not on the device."""
    on_gpu = [t.device for t in tensors if t.device.type == "cuda"]
    if device is not None:
        dev = torch.device(device)
    elif on_gpu:
        dev = on_gpu[0]
    else:
        dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
    if dev.type != "cuda":
        raise RuntimeError(no_gpu)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    if any(d != dev for d in on_gpu):
        raise ValueError(mixed)
    host = [i for i, t in enumerate(tensors) if t.device.type != "cuda"]
    items = [t if t.device.type != "cuda" else t.to(torch.float32).contiguous() for t in tensors]
    if host:
        down = torch.cat([items[i].to(torch.float32).reshape(-1) for i in host]).to(dev)
        for i, piece in zip(host, down.split([items[i].numel() for i in host])):
            items[i] = piece
    base = min(t.data_ptr() for t in items)
    return items, dev, base, (C.c_int64 * len(items))(*[(t.data_ptr() - base) // 4 for t in items])


def flat_segments(tables):
    """Per-item lists of (dst, src, frames) as the entry points take them: (counts int32[B], flat triples int32[3 * total]), ctypes."""
    flat = [int(v) for t in tables for seg in t for v in seg]
    return (C.c_int32 * len(tables))(*[len(t) for t in tables]), (C.c_int32 * max(len(flat), 1))(*flat)


def wave_crossfade(wav: torch.Tensor, lens: list[int], cross_fade_samples: int) -> torch.Tensor:
    """cross_fade_concat on the device (f5_wave_crossfade): piece i is wav[i, :lens[i]] of an f32 [B, stride] device tensor,
    B <= 64; returns f32[total], bit for bit cross_fade_concat(pieces, ...).astype(float32).  One launch, no synchronisation."""
    if wav.device.type != "cuda":
        raise RuntimeError("the HIP cross-fade only runs on a GPU (there is no CPU path: cross_fade_concat is the host form)")
    if wav.dim() != 2 or wav.dtype != torch.float32 or wav.stride(1) != 1 or len(lens) != wav.shape[0]:
        raise ValueError("wave_crossfade: wav must be f32 [B, stride] with unit element stride and one length per row")
    total = cross_fade_plan(lens, cross_fade_samples)[2]
    out = torch.empty(total, device=wav.device, dtype=torch.float32)
    n = C.c_int64()
    with torch.cuda.device(wav.device):
        _lib.check(_lib.load().f5_wave_crossfade(_ptr(wav), wav.shape[0], wav.stride(0), _lib.int_array(lens), int(cross_fade_samples),
                                                 _ptr(out), total, C.byref(n), _stream_ptr(wav.device)), "f5_wave_crossfade")
    assert n.value == total
    return out


def cross_fade_plan(lens: list[int], cross_fade_samples: int) -> tuple[list[int], list[int], int]:
    """The integer plan of cross_fade_concat's left fold (the arithmetic f5_wave_crossfade does on the host): piece i starts at
    offs[i] of the result and its first ns[i] samples fade in over what is already there; returns (offs, ns, total).
    n_i = min(cross_fade_samples, length so far, len_i), 0 for the first piece and when cross_fade_samples <= 0."""
    offs, ns, total = [], [], 0
    for i, ln in enumerate(lens):
        n = min(cross_fade_samples, total, ln) if i > 0 and cross_fade_samples > 0 else 0
        offs.append(total - n)
        ns.append(n)
        total = offs[-1] + ln
    return offs, ns, total


def _placed(items, who):
    """(device, base, starts) of items that are on the device already."""
    return ragged_items(items, None, f"{who} only runs on a GPU (there is no CPU path)", f"{who}: the items are on different devices")[1:]


def join_plan(lens: list[int], fades: list[int]) -> tuple[list[int], list[int], int]:
    """cross_fade_plan with a fade request per piece (the arithmetic f5_wave_join does on the host): piece 0 and every piece with
    fades[i] == 0 open a run, placed behind everything before it; any other piece fades in over n_i = min(fades[i], length of its
    run so far, len_i) samples.  The running length restarts with every run, so a run is placed exactly as cross_fade_plan places
    it alone.  Returns (offs, ns, total)."""
    if len(lens) != len(fades):
        raise ValueError(f"join_plan: {len(lens)} lengths for {len(fades)} fades (need one fade per piece)")
    offs, ns, total, run = [], [], 0, 0
    for i, (ln, fade) in enumerate(zip(lens, fades)):
        opens = i == 0 or fade == 0
        n = 0 if opens else min(fade, run, ln)
        offs.append(total - n)
        ns.append(n)
        total = offs[-1] + ln
        run = ln if opens else run - n + ln
    return offs, ns, total


def wave_join(items, fades) -> torch.Tensor:
    """The pieces of a multi-voice script as one waveform (f5_wave_join; the contract is in include/f5_hip.h): items are 1-D f32
    device tensors with unit stride, read where they lie (rows of several decode_ragged results, in any order), fades[i] >= 0 the
    cross-fade in samples into what stands in front of piece i (0: plain concatenation, the piece opens a run).  Returns f32[total],
    bit for bit np.concatenate([cross_fade_concat(run) for every run]).astype(float32).  One launch, no synchronisation; at most
    65535 pieces."""
    items, fades = list(items), [int(f) for f in fades]
    if not items or len(items) != len(fades):
        raise ValueError(f"wave_join: {len(items)} pieces for {len(fades)} fades (need one fade per piece, at least one piece)")
    if any(t.dim() != 1 or t.dtype != torch.float32 or t.shape[0] < 1 or t.stride(0) != 1 for t in items):
        raise ValueError("wave_join: every piece must be a 1-D f32 tensor with unit stride and at least one sample")
    if any(t.device.type != "cuda" for t in items):
        raise RuntimeError("wave_join only runs on a GPU (there is no CPU path: cross_fade_concat per run is the host form)")
    lens = [int(t.shape[0]) for t in items]
    dev, base, starts = _placed(items, "wave_join")
    total = join_plan(lens, fades)[2]
    out = torch.empty(total, device=dev, dtype=torch.float32)
    n = C.c_int64()
    with torch.cuda.device(dev):
        _lib.check(_lib.load().f5_wave_join(C.c_void_p(base), len(items), starts, _lib.int_array(lens), _lib.int_array(fades), _ptr(out),
                                            total, C.byref(n), _stream_ptr(dev)), "f5_wave_join")
    assert n.value == total
    return out


def deliver_plan(out_rate: int, n: int, final: bool = True) -> tuple[int, int]:
    """(len, ready) of a 24 kHz stream of n samples at out_rate (f5_wave_deliver_plan, pure host arithmetic): its length
    there, and how many leading output samples are settled -- all of them once the stream is final, else those whose taps lie
    inside the n samples.  A settled sample never changes as the stream grows."""
    ln, ready = C.c_int64(), C.c_int64()
    _lib.check(_lib.load().f5_wave_deliver_plan(int(out_rate), int(n), int(bool(final)), C.byref(ln), C.byref(ready)),
               "f5_wave_deliver_plan")
    return ln.value, ready.value


def _deliver_bank(lib, h, dev, out_rate: int):
    """The (24000 -> out_rate) filter bank in the handle h: uploaded on the rate's first use (which synchronises once), inside a
    `torch.cuda.device(dev)` block."""
    from .mel import _resample_bank_f32

    known = h.__dict__.setdefault("_deliver_banks", set())
    if out_rate != 24_000 and out_rate not in known:
        deliver_plan(out_rate, 0)                                         # (refuses the rate before a bank is built for it)
        bank = _resample_bank_f32(24_000, out_rate)
        _lib.check(lib.f5_mel_resample_bank(h, 24_000, out_rate, C.c_void_p(bank.data_ptr()), bank.numel(), _stream_ptr(dev)),
                   "f5_mel_resample_bank")
        known.add(out_rate)


def emit_plan(streams) -> tuple[list[int], int]:
    """Where f5_wave_emit puts every stream: (byte offset per stream, bytes in all) -- the running byte total rounded up to 16 in
    front of every stream, 4 bytes per f32 sample and 2 per s16 sample of its range."""
    starts, run = [], 0
    for st in streams:
        o0, o1 = st["range"]
        run = (run + 15) // 16 * 16
        starts.append(run)
        run += max(int(o1) - int(o0), 0) * (4 if _lib.PCM_FORMATS[st["sample_format"]] == _lib.F5_PCM_F32 else 2)
    return starts, run


def wave_emit(mel_spec, streams):
    """Join and delivery for many streams in ONE launch (f5_wave_emit; the contract is in include/f5_hip.h): what a server tick
    sends to its clients.  Every stream is a dict:
      pieces         1-D f32 device tensors at 24 kHz with unit stride, read where they lie (wave_join's items);
      fades          one per piece, the cross-fade in samples into what stands in front of it (0 opens a run);
      settled        how many leading samples of the joined stream are delivered (0 .. join_plan's total);
      final          whether the stream ends at `settled`;
      range          (o0, o1): the output samples wanted, inside [0, ready] of deliver_plan(out_rate, settled, final);
      out_rate, sample_format ("f32" / "s16"): the client's, each stream its own.
    Returns (views, buffer): `buffer` one uint8 device tensor and views[s] stream s's samples in it, typed f32 or int16 -- bit for bit
    wave_deliver(wave_join(pieces, fades)[:settled], ...) of that stream alone, without the joined waveform ever being written.
    One copy of `buffer` brings every stream to the host; stream s's bytes start at emit_plan's offset.  The bank of a new rate is
    uploaded on its first use (which synchronises once); otherwise one launch and no synchronisation.  At most 65535 streams and
    65535 pieces in all."""
    streams = list(streams)
    if not streams:
        raise ValueError("wave_emit: no stream")
    if mel_spec.target_sample_rate != 24_000:
        raise ValueError(f"wave_emit: the stage reads 24 kHz audio; this MelSpec runs at {mel_spec.target_sample_rate} Hz")
    pieces, counts = [], []
    for s, st in enumerate(streams):
        if st["sample_format"] not in _lib.PCM_FORMATS:
            raise ValueError(f"wave_emit: stream {s}: sample_format {st['sample_format']!r} (expected one of {sorted(_lib.PCM_FORMATS)})")
        own = list(st["pieces"])
        if not own or len(own) != len(st["fades"]):
            raise ValueError(f"wave_emit: stream {s}: {len(own)} pieces for {len(st['fades'])} fades (need one fade per piece, at least "
                             "one piece)")
        pieces += own
        counts.append(len(own))
    if any(t.dim() != 1 or t.dtype != torch.float32 or t.shape[0] < 1 or t.stride(0) != 1 for t in pieces):
        raise ValueError("wave_emit: every piece must be a 1-D f32 tensor with unit stride and at least one sample")
    if any(t.device.type != "cuda" for t in pieces):
        raise RuntimeError("wave_emit only runs on a GPU (there is no CPU path)")
    S = len(streams)
    dev, base, starts = _placed(pieces, "wave_emit")
    at, total = emit_plan(streams)
    out = torch.empty(max(total, 1), device=dev, dtype=torch.uint8)
    lib, h = _lib.load(), mel_spec._handle(dev)
    got = (C.c_int64 * S)()
    i64 = lambda vals: (C.c_int64 * S)(*[int(v) for v in vals])   # noqa: E731
    with torch.cuda.device(dev):
        for rate in sorted({int(st["out_rate"]) for st in streams}):
            _deliver_bank(lib, h, dev, rate)
        _lib.check(lib.f5_wave_emit(h, C.c_void_p(base), S, _lib.int_array(counts), starts, _lib.int_array([t.shape[0] for t in pieces]),
                                    _lib.int_array([f for st in streams for f in st["fades"]]), i64(st["settled"] for st in streams),
                                    _lib.int_array([bool(st["final"]) for st in streams]), i64(st["range"][0] for st in streams),
                                    i64(st["range"][1] for st in streams), _lib.int_array([st["out_rate"] for st in streams]),
                                    _lib.int_array([_lib.PCM_FORMATS[st["sample_format"]] for st in streams]), _ptr(out), total, got,
                                    _stream_ptr(dev)), "f5_wave_emit")
    assert list(got) == at
    views = []
    for a, st in zip(at, streams):
        f32 = _lib.PCM_FORMATS[st["sample_format"]] == _lib.F5_PCM_F32
        count = max(int(st["range"][1]) - int(st["range"][0]), 0)
        views.append(out[a:a + count * (4 if f32 else 2)].view(torch.float32 if f32 else torch.int16))
    return views, out


def wave_deliver(mel_spec, items, *, out_rate: int, sample_format: str = "f32", ranges=None, final=True):
    """Generated audio at a client's rate and sample format (f5_wave_deliver; the contract is in include/f5_hip.h): items are 1-D
    f32 device tensors at 24 kHz with unit stride, read where they lie; `final` (one bool, or one per item) says whether an item
    is a finished stream or the part of a growing one that exists so far; ranges[i] = (o0, o1) the output samples wanted, inside
    [0, ready] of deliver_plan (None: everything that is settled).  mel_spec: the model's MelSpec, whose handle keeps the
    (24000 -> out_rate) filter bank (the bank of a new rate is uploaded on its first use, which synchronises once).  Returns one
    device tensor per item, f32 or int16 (sample_format "f32" / "s16": the 16-bit view of generated audio, y * 32767 rounded to
    nearest even and clamped), views of one packed buffer.  One launch, no synchronisation; at most 65535 items."""
    items = list(items)
    if not items:
        raise ValueError("wave_deliver: no item")
    if sample_format not in _lib.PCM_FORMATS:
        raise ValueError(f"wave_deliver: sample_format {sample_format!r} (expected one of {sorted(_lib.PCM_FORMATS)})")
    if mel_spec.target_sample_rate != 24_000:
        raise ValueError(f"wave_deliver: the stage reads 24 kHz audio; this MelSpec runs at {mel_spec.target_sample_rate} Hz")
    if any(t.dim() != 1 or t.dtype != torch.float32 or t.shape[0] < 1 or t.stride(0) != 1 for t in items):
        raise ValueError("wave_deliver: every item must be a 1-D f32 tensor with unit stride and at least one sample")
    if any(t.device.type != "cuda" for t in items):
        raise RuntimeError("wave_deliver only runs on a GPU (there is no CPU path)")
    B, out_rate = len(items), int(out_rate)
    finals = [bool(final)] * B if isinstance(final, (bool, int)) else [bool(f) for f in final]
    if len(finals) != B or (ranges is not None and len(ranges) != B):
        raise ValueError(f"wave_deliver: {B} items need one `final` flag and one range each")
    ns = [int(t.shape[0]) for t in items]
    if ranges is None:
        ranges = [(0, deliver_plan(out_rate, n, f)[1]) for n, f in zip(ns, finals)]
    dev, base, starts = _placed(items, "wave_deliver")
    fmt = _lib.PCM_FORMATS[sample_format]
    per16 = 4 if fmt == _lib.F5_PCM_F32 else 8
    total = 0
    for o0, o1 in ranges:
        total = (total + per16 - 1) // per16 * per16 + max(int(o1) - int(o0), 0)
    out = torch.empty(max(total, 1), device=dev, dtype=torch.float32 if fmt == _lib.F5_PCM_F32 else torch.int16)
    lib, h = _lib.load(), mel_spec._handle(dev)
    at = (C.c_int64 * B)()
    with torch.cuda.device(dev):
        _deliver_bank(lib, h, dev, out_rate)
        _lib.check(lib.f5_wave_deliver(h, C.c_void_p(base), B, starts, _lib.int_array(ns), _lib.int_array(finals),
                                       (C.c_int64 * B)(*[int(o0) for o0, _ in ranges]), (C.c_int64 * B)(*[int(o1) for _, o1 in ranges]),
                                       out_rate, fmt, _ptr(out), total, at, _stream_ptr(dev)), "f5_wave_deliver")
    return [out[a:a + int(o1) - int(o0)] for a, (o0, o1) in zip(at, ranges)]


def silence_flags(items, shapes, rates, lens_ms, queries, qscale, tables=None):
    """One f5_silence_analyse over a ragged batch and ONE small device-to-host read: items are contiguous f32 device tensors
    holding [C_i, F_i] = shapes[i], lens_ms the length in ms of each analysed signal, queries (W, s, T, kind) tuples
    (include/f5_hip.h), tables per item the (dst, src, frames) segments the item is read through (None: as it lies).
    Returns flags[i][k]: a uint8 numpy array per item and query."""
    lib, B, nq = _lib.load(), len(items), len(queries)
    dev, base, starts = _placed(items, "silence_flags")
    q_arr = _lib.int_array([v for q in queries for v in q])
    len_arr = _lib.int_array(lens_ms)
    counts, offs, total = (C.c_int32 * (B * nq))(), (C.c_int64 * (B * nq))(), C.c_int64()
    _lib.check(lib.f5_silence_plan(B, len_arr, nq, q_arr, counts, offs, C.byref(total)), "f5_silence_plan")
    flags = torch.empty(max(total.value, 1), device=dev, dtype=torch.uint8)
    seg_counts, seg_flat = flat_segments(tables) if tables is not None else (None, None)
    with torch.cuda.device(dev):
        _lib.check(lib.f5_silence_analyse(C.c_void_p(base), B, starts, _lib.int_array([c for c, _ in shapes]),
                                          _lib.int_array([f for _, f in shapes]), _lib.int_array(rates), len_arr, float(qscale), nq, q_arr,
                                          seg_counts, seg_flat, _ptr(flags), total.value, _stream_ptr(dev)), "f5_silence_analyse")
    host = flags.cpu().numpy()
    return [[host[offs[b * nq + k]:offs[b * nq + k] + counts[b * nq + k]] for k in range(nq)] for b in range(B)]


def wave_gather(items, shapes, tables, out_frames, qscale):
    """One f5_wave_gather: item i read through tables[i] into [C_i, out_frames[i]] of one packed device buffer (every item starts
    on a 16-byte multiple).  Returns the views."""
    B = len(items)
    dev, base, starts = _placed(items, "wave_gather")
    offs, run = [], 0
    for (c, _), n in zip(shapes, out_frames):
        run = (run + 3) // 4 * 4
        offs.append(run)
        run += c * n
    out = torch.empty(max(run, 1), device=dev, dtype=torch.float32)
    seg_counts, seg_flat = flat_segments(tables)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().f5_wave_gather(C.c_void_p(base), B, starts, _lib.int_array([c for c, _ in shapes]),
                                              _lib.int_array([f for _, f in shapes]), float(qscale), seg_counts, seg_flat,
                                              _lib.int_array(out_frames), (C.c_int64 * B)(*offs), _ptr(out), run, _stream_ptr(dev)),
                   "f5_wave_gather")
    return [out[o:o + c * n].view(c, n) for o, (c, _), n in zip(offs, shapes, out_frames)]


def wave_splice(wav: torch.Tensor, wav_lens, originals, plans, cross_fade_samples: int, hop: int = HOP_LENGTH) -> torch.Tensor:
    """The original recording outside the edited spans (f5_wave_splice; the contract is in include/f5_hip.h): wav f32 [B, stride]
    on a GPU with item b in wav[b, :wav_lens[b]] (decode_ragged's return), originals the prepared recordings as 1-D f32 device
    tensors at the model's rate (normalise_prompt / prepare_ragged; read where they are), plans edit_plan's return per item.
    Every KEEP segment's samples become the original's, cross-faded linearly over min(cross_fade_samples, half the segment)
    samples at each end that is not an end of the waveform; everything else is wav's, +0.0 behind wav_lens[b].  Returns a new
    tensor of wav's shape.  One launch, no synchronisation; at most 64 items."""
    if wav.device.type != "cuda":
        raise RuntimeError("the HIP waveform splice only runs on a GPU (there is no CPU path)")
    B = wav.shape[0] if wav.dim() == 2 else -1
    wav_lens, originals, plans = [int(n) for n in wav_lens], list(originals), list(plans)
    if B < 0 or wav.dtype != torch.float32 or wav.stride(1) != 1 or not len(wav_lens) == len(originals) == len(plans) == B:
        raise ValueError("wave_splice: wav must be f32 [B, stride] with unit element stride, with one length, one original and one "
                         "plan per row")
    mixed = "wave_splice: every original must be a 1-D tensor on wav's device"
    if any(a.dim() != 1 or a.device != wav.device for a in originals):
        raise ValueError(mixed)
    originals, dev, base, starts = ragged_items(originals, wav.device, mixed, mixed)
    counts, flat = segment_table(plans, keep_only=True)
    out = torch.empty(wav.shape, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().f5_wave_splice(_ptr(wav), B, wav.stride(0), _lib.int_array(wav_lens), C.c_void_p(base), starts,
                                              _lib.int_array([a.shape[0] for a in originals]), counts, flat, int(hop),
                                              int(cross_fade_samples), _ptr(out), out.stride(0), _stream_ptr(dev)), "f5_wave_splice")
    return out
