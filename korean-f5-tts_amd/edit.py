"""Host arithmetic of speech editing (the reference's infer/speech_edit.py:157-195): from the spans to replace, in seconds, to
the segments of the edited timeline in mel frames, and from there to the edit mask CFM.sample takes.  Pure Python / host torch: the
data movement is libf5hip's (csrc/edit.hip, through MelSpec.edit_assemble and wave.wave_splice)."""
from __future__ import annotations

import torch

MAX_PARTS = 16     # spans of one recording: 17 KEEP and 16 EDIT segments at most, what f5_edit_assemble takes per item
MAX_ITEMS = 64     # recordings of one f5_edit_assemble / f5_wave_splice call


def edit_plan(n_frames: int, parts_to_edit, fix_duration=None, *, sample_rate: int = 24000, hop_length: int = 256):
    """The frame arithmetic of speech_edit.py:157-195 for one recording of `n_frames` mel frames: parts_to_edit is a list of
    (start, end) in seconds, in time order; fix_duration, where given, the new length in seconds of each part.
    Returns (segments, D): segments is a list of (dst_frame, src_frame, frames) over the edited timeline of D frames --
    src_frame >= 0: a KEEP segment, the original's frames [src_frame, src_frame + frames); src_frame = -1: an EDIT segment of
    zero frames that sample() fills in.  Zero-length segments are dropped.  Frame numbers are Python's round() (ties to even) of
    `seconds * sample_rate / hop_length`, exactly as the script writes it.
    Where the script slices silently (its mel and mask then disagree in length) this raises ValueError: a part that starts before
    the previous one ends, ends before it starts or ends behind the recording; a fix_duration list of another length than
    parts_to_edit, or a negative one; more than 16 parts; a result of fewer than 2 frames."""
    parts = [tuple(p) for p in parts_to_edit]
    n_frames = int(n_frames)
    if len(parts) > MAX_PARTS:
        raise ValueError(f"edit_plan: {len(parts)} parts to edit; at most {MAX_PARTS} per recording")
    if any(len(p) != 2 for p in parts):
        raise ValueError("edit_plan: every part is (start, end) in seconds")
    if fix_duration is not None and len(fix_duration) != len(parts):
        raise ValueError(f"edit_plan: {len(fix_duration)} fix_duration values for {len(parts)} parts (need one per part)")
    if n_frames < 0:
        raise ValueError(f"edit_plan: n_frames = {n_frames}")
    segments, offset, dst = [], 0, 0

    def emit(src, frames):
        nonlocal dst
        if frames > 0:
            segments.append((dst, src, frames))
            dst += frames

    for k, (start, end) in enumerate(parts):
        dur = end - start if fix_duration is None else fix_duration[k]
        start_frame = round(start * sample_rate / hop_length)
        end_frame = round(end * sample_rate / hop_length)
        part_frames = round(dur * sample_rate / hop_length)
        if not offset <= start_frame <= end_frame <= n_frames:
            raise ValueError(f"edit_plan: part {k} ({start} s, {end} s) is frames [{start_frame}, {end_frame}); need "
                             f"{offset} <= start <= end <= {n_frames} (parts in time order, inside the recording)")
        if part_frames < 0:
            raise ValueError(f"edit_plan: part {k} would last {part_frames} frames")
        emit(offset, start_frame - offset)
        emit(-1, part_frames)
        offset = end_frame
    emit(offset, n_frames - offset)
    if dst < 2:
        raise ValueError(f"edit_plan: the edited recording has {dst} frames; need at least 2")
    return segments, dst


def edit_mask(plans) -> torch.Tensor:
    """CFM.sample's edit_mask for a batch of plans (edit_plan's returns): bool [B, D_max] on the host, True = keep the frame of
    `cond`, False over every EDIT segment; True behind D_i, as the script pads (speech_edit.py:195; sample() cuts it with lens)."""
    plans = list(plans)
    mask = torch.ones(len(plans), max(D for _, D in plans), dtype=torch.bool)
    for b, (segments, _D) in enumerate(plans):
        for dst, src, frames in segments:
            if src < 0:
                mask[b, dst:dst + frames] = False
    return mask


def segment_table(plans, keep_only: bool = False):
    """(counts per item, flat [dst, src, frames, ...]) as f5_edit_assemble / f5_wave_splice take them (wave.flat_segments);
    keep_only: without the EDIT segments."""
    from .wave import flat_segments   # (wave.py imports this module)

    return flat_segments([[s for s in segments if s[1] >= 0 or not keep_only] for segments, _D in plans])
