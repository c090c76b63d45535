"""Host arithmetic of silence clipping: pydub 0.25's `silence` module (detect_silence, detect_nonsilent, split_on_silence,
detect_leading_silence) and the reference's use of it (infer/utils_infer.py:348-361 remove_silence_edges, :385-419 the 12 s prompt
clip, :784-793 remove_silence_for_generated_wav), restated from their documented behaviour on top of the per-window flags that
libf5hip computes (csrc/silence.hip; the arithmetic contract is in include/f5_hip.h).  Pure Python: no torch and no audio on the
decision path -- flags in, frame ranges out.  pydub is not installed, so parity with pydub itself is unpinned.

Units: `ms` positions live on an item's millisecond grid, pos(R, ms) = (R * ms) // 1000 frames; a signal's length in ms is
ms_len(frames, R) = round(1000 * (frames / R)), Python's round on that float.  A *signal* is a list of pieces (src, frames) of an
item, src = -1 for frames of silence (what pydub pads a slice with when it reaches past the data)."""
from __future__ import annotations

import math

MIN_RATE, MAX_RATE = 11025, 384000          # below 11025 Hz pydub's silent() segments would resample the prompt up (not built)
PROMPT_QSCALE, WAVE_QSCALE = 32768.0, 32767.0
KIND_SILENCE, KIND_CHUNKS = 0, 1


def pos(rate: int, ms: int) -> int:
    return (rate * ms) // 1000


def ms_len(frames: int, rate: int) -> int:
    return round(1000 * (frames / rate))


def rms_threshold(db: float) -> int:
    """detect_silence's `rms <= db_to_float(db) * 32768` for the integer rms audioop returns: rms <= T."""
    return math.floor(10 ** (db / 20) * 32768)


def dbfs_threshold(db: float) -> int:
    """The largest integer rms r with 20 * log10(r / 32768) < db (the edge trim's `dBFS` tests; rms 0 is -inf)."""
    r = max(int(10 ** (db / 20) * 32768) + 2, 1)
    while r > 0 and not 20 * math.log(r / 32768, 10) < db:
        r -= 1
    return r


CLIP_QUERIES = ((1000, 10, rms_threshold(-50), KIND_SILENCE), (100, 10, rms_threshold(-40), KIND_SILENCE))
EDGE_QUERIES = ((10, 10, dbfs_threshold(-42), KIND_CHUNKS), (1, 1, dbfs_threshold(-42), KIND_CHUNKS))
REMOVE_QUERIES = ((1000, 10, rms_threshold(-50), KIND_SILENCE),)


def query_starts(L: int, W: int, s: int, kind: int = KIND_SILENCE) -> list[int]:
    """The window starts of a query, in the order of its flags."""
    if kind == KIND_CHUNKS:
        return list(range(0, L, s))
    if L < W:
        return []
    last = L - W
    starts = list(range(0, last + 1, s))
    if last % s:
        starts.append(last)
    return starts


def silent_ranges(flags, L: int, W: int, s: int) -> list[list[int]]:
    """detect_silence from its flags: the silent starts merged into [start, end] ranges in ms."""
    hits = [a for a, f in zip(query_starts(L, W, s), flags) if f]
    if not hits:
        return []
    ranges, prev, start = [], hits[0], hits[0]
    for a in hits[1:]:
        if a != prev + s and a > prev + W:
            ranges.append([start, prev + W])
            start = a
        prev = a
    ranges.append([start, prev + W])
    return ranges


def nonsilent_ranges(silent, L: int) -> list[list[int]]:
    """detect_nonsilent: the complement of the silent ranges in [0, L]."""
    if not silent:
        return [[0, L]]
    if silent[0][0] == 0 and silent[0][1] == L:
        return []
    out, prev_end = [], 0
    for a, b in silent:
        out.append([prev_end, a])
        prev_end = b
    if silent[-1][1] != L:
        out.append([prev_end, L])
    if out[0] == [0, 0]:
        out.pop(0)
    return out


def split_ranges(nonsilent, L: int, keep_silence: int) -> list[list[int]]:
    """split_on_silence's output ranges: widened by keep_silence, neighbours that then overlap meet half way, clipped to [0, L]."""
    out = [[a - keep_silence, b + keep_silence] for a, b in nonsilent]
    for cur, nxt in zip(out, out[1:]):
        if nxt[0] < cur[1]:
            cur[1] = (cur[1] + nxt[0]) // 2
            nxt[0] = cur[1]
    return [[max(a, 0), min(b, L)] for a, b in out]


def split_on_silence(flags, L: int, W: int, s: int, keep_silence: int) -> list[list[int]]:
    return split_ranges(nonsilent_ranges(silent_ranges(flags, L, W, s), L), L, keep_silence)


# ------------------------------------------------------------------------------------------------------------- signals
def signal_frames(pieces) -> int:
    return sum(n for _, n in pieces)


def slice_item(frames: int, rate: int, a: int, b: int):
    """item[a:b] in ms as one piece list: frames [pos(a), pos(b)), the part at or past `frames` as silence."""
    f0, f1 = pos(rate, a), pos(rate, b)
    have = max(min(f1, frames) - f0, 0)
    out = [(f0, have)] if have else []
    if f1 - f0 - have > 0:
        out.append((-1, f1 - f0 - have))
    return out


def slice_signal(pieces, f0: int, f1: int):
    """Frames [f0, f1) of a signal; what lies past its end is silence."""
    out, at = [], 0
    for src, n in pieces:
        lo, hi = max(f0, at), min(f1, at + n)
        if lo < hi:
            out.append((src + (lo - at) if src >= 0 else -1, hi - lo))
        at += n
    if f1 > max(at, f0):
        out.append((-1, f1 - max(at, f0)))
    return out


def segment_table(pieces):
    """(dst, src, frames) triples of a signal as f5_silence_analyse / f5_wave_gather take them; silence is left uncovered."""
    table, dst = [], 0
    for src, n in pieces:
        if src >= 0 and n > 0:
            if table and table[-1][0] + table[-1][2] == dst and table[-1][1] + table[-1][2] == src:
                table[-1] = (table[-1][0], table[-1][1], table[-1][2] + n)
            else:
                table.append((dst, src, n))
        dst += n
    return table


# ------------------------------------------------------------------------------------------------------------- the plans
def _collect(ranges, frames: int, rate: int):
    """The reference's loop over the non-silent segments (utils_infer.py:391-396): append until more than 6 s are there and the
    next segment would take the result over 12 s."""
    pieces, total = [], 0
    for a, b in ranges:
        seg = slice_item(frames, rate, a, b)
        n = signal_frames(seg)
        if ms_len(total, rate) > 6000 and ms_len(total + n, rate) > 12000:
            return pieces, True
        pieces += seg
        total += n
    return pieces, False


def prompt_clip_plan(flags_long, flags_short, frames: int, rate: int):
    """The three clipping rules of preprocess_ref_audio_text (utils_infer.py:387-415) for one prompt of `frames` frames at `rate`
    Hz, from the flags of CLIP_QUERIES[0] and CLIP_QUERIES[1]: returns (pieces of the clipped signal, the rule whose
    "clipping short" message the reference would print: 0 none, 1, 2 or 3)."""
    L = ms_len(frames, rate)
    W, s, _, _ = CLIP_QUERIES[0]
    pieces, cut = _collect(split_on_silence(flags_long, L, W, s, 1000), frames, rate)
    rule = 1 if cut else 0
    if ms_len(signal_frames(pieces), rate) > 12000:
        W, s, _, _ = CLIP_QUERIES[1]
        pieces, cut = _collect(split_on_silence(flags_short, L, W, s, 1000), frames, rate)
        rule = 2 if cut else 0
    if ms_len(signal_frames(pieces), rate) > 12000:
        pieces = slice_signal(pieces, 0, pos(rate, 12000))
        rule = 3
    return pieces, rule


def leading_trim(flags_chunks, L: int) -> int:
    """detect_leading_silence(chunk_size=10) from the flags of EDGE_QUERIES[0]: the ms to drop in front."""
    k = 0
    for f in flags_chunks:
        if not f:
            break
        k += 1
    return min(10 * k, L)


def after_lead(pieces, rate: int, lead: int):
    """audio[lead:] of a signal: (its pieces, whether its millisecond grid is the signal's own shifted by `lead` -- then the
    per-millisecond flags of the signal serve it, else it needs flags of its own)."""
    total = signal_frames(pieces)
    L = ms_len(total, rate)
    rest = slice_signal(pieces, pos(rate, lead), pos(rate, L))
    same_grid = (rate * lead) % 1000 == 0 and ms_len(signal_frames(rest), rate) == L - lead
    return rest, same_grid


def trailing_cut(flags_ms, frames: int, rate: int) -> int:
    """The loop of remove_silence_edges (utils_infer.py:354-359) over a signal of `frames` frames, from its per-millisecond flags
    (EDGE_QUERIES[1]): 0.001 is taken off the float duration once per silent trailing millisecond, in that order; returns the ms
    to keep."""
    L = ms_len(frames, rate)
    duration = frames / rate if frames else 0.0
    for i in reversed(range(L)):
        if not flags_ms[i]:
            break
        duration -= 0.001
    return min(max(int(duration * 1000), 0), L)


def silent_tail_frames(rate: int) -> int:
    """Frames of `AudioSegment.silent(duration=50)` once pydub has brought it to `rate`: 551 frames at 11025 Hz through
    audioop.ratecv."""
    return (550 * rate) // 11025 + 1


def finish_prompt(rest, keep_ms: int, rate: int):
    """(pieces, frames) of `audio[:keep_ms] + silent(50)` for the signal behind the leading trim."""
    body = slice_signal(rest, 0, pos(rate, keep_ms))
    tail = silent_tail_frames(rate)
    return body + [(-1, tail)], signal_frames(body) + tail


def remove_silence_plan(flags, frames: int, rate: int):
    """remove_silence_for_generated_wav (utils_infer.py:784-793): the non-silent segments, 500 ms kept around each, concatenated."""
    L = ms_len(frames, rate)
    W, s, _, _ = REMOVE_QUERIES[0]
    pieces = []
    for a, b in split_on_silence(flags, L, W, s, 500):
        pieces += slice_item(frames, rate, a, b)
    return pieces
