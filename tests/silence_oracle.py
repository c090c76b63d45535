"""The yardstick of the silence-clipping tests: pydub 0.25's AudioSegment slicing and `silence` module, and the reference's use of
them (infer/utils_infer.py:348-361, 385-419, 784-793), written literally, slice by slice, on 16-bit samples, with `audioop.rms`
(the C routine pydub itself calls) and the float dB comparisons as pydub writes them.  It shares no code with the package's
silence.py and never looks at flags or prefix sums: every decision is an rms of a slice.

One deviation from pydub's text, stated by the contract in include/f5_hip.h: a millisecond position is the frame
(rate * ms) // 1000 in integers, where pydub computes int(ms * (rate / 1000.0)) in floats.  pydub is not installed, so parity with
pydub itself is unpinned."""
import itertools
import math

import numpy as np
import pytest

audioop = pytest.importorskip("audioop")


def db_to_float(db):
    return 10 ** (db / 20)


def ratio_to_db(ratio):
    if ratio == 0:
        return -float("inf")
    return 20 * math.log(ratio, 10)


class Segment:
    """An AudioSegment of 16-bit samples: `data` holds interleaved int16 frames as bytes."""
    sample_width = 2
    max_possible_amplitude = 32768

    def __init__(self, data: bytes, rate: int, channels: int):
        self.data, self.rate, self.channels = bytes(data), int(rate), int(channels)
        self.frame_width = self.sample_width * self.channels

    @classmethod
    def from_array(cls, q: np.ndarray, rate: int):
        """q: int16 [channels, frames]."""
        q = np.asarray(q, dtype=np.int16)
        return cls(np.ascontiguousarray(q.T).tobytes(), rate, q.shape[0])

    @classmethod
    def silent(cls, duration=1000, frame_rate=11025):
        frames = int(frame_rate * (duration / 1000.0))
        return cls(b"\0\0" * frames, frame_rate, 1)

    def array(self) -> np.ndarray:
        """int16 [channels, frames]."""
        return np.frombuffer(self.data, dtype=np.int16).reshape(self.frame_count(), self.channels).T.copy()

    def _spawn(self, data, rate=None, channels=None):
        return Segment(data, self.rate if rate is None else rate, self.channels if channels is None else channels)

    def frame_count(self, ms=None):
        if ms is not None:
            return (self.rate * ms) // 1000
        return len(self.data) // self.frame_width

    def __len__(self):
        return round(1000 * (self.frame_count() / self.rate))

    @property
    def duration_seconds(self):
        return self.frame_count() and self.frame_count() / self.rate or 0.0

    @property
    def rms(self):
        return audioop.rms(self.data, self.sample_width)

    @property
    def dBFS(self):
        rms = self.rms
        if not rms:
            return -float("inf")
        return ratio_to_db(rms / self.max_possible_amplitude)

    def __getitem__(self, millisecond):
        if isinstance(millisecond, slice):
            start = millisecond.start if millisecond.start is not None else 0
            end = millisecond.stop if millisecond.stop is not None else len(self)
            start = min(start, len(self))
            end = min(end, len(self))
        else:
            start = millisecond
            end = millisecond + 1
        start = self.frame_count(ms=start) * self.frame_width
        end = self.frame_count(ms=end) * self.frame_width
        data = self.data[start:end]
        expected_length = end - start
        missing_frames = (expected_length - len(data)) // self.frame_width
        if missing_frames:
            assert missing_frames <= self.frame_count(ms=2), "TooManyMissingFrames"
            data += b"\0" * (missing_frames * self.frame_width)
        return self._spawn(data)

    def set_frame_rate(self, frame_rate):
        if frame_rate == self.rate:
            return self
        converted = audioop.ratecv(self.data, self.sample_width, self.channels, self.rate, frame_rate, None)[0] if self.data else b""
        return self._spawn(converted, rate=frame_rate)

    def set_channels(self, channels):
        if channels == self.channels:
            return self
        assert self.channels == 1, "only mono is ever widened here"
        mono = np.frombuffer(self.data, dtype=np.int16)
        return self._spawn(np.repeat(mono, channels).tobytes(), channels=channels)

    def __add__(self, other):
        channels, rate = max(self.channels, other.channels), max(self.rate, other.rate)
        a = self.set_frame_rate(rate).set_channels(channels)
        b = other.set_frame_rate(rate).set_channels(channels)
        return a._spawn(a.data + b.data)


# ------------------------------------------------------------------------------------------------------- pydub.silence
def detect_silence(audio_segment, min_silence_len=1000, silence_thresh=-16, seek_step=1):
    seg_len = len(audio_segment)
    if seg_len < min_silence_len:
        return []
    silence_thresh = db_to_float(silence_thresh) * audio_segment.max_possible_amplitude
    silence_starts = []
    last_slice_start = seg_len - min_silence_len
    slice_starts = range(0, last_slice_start + 1, seek_step)
    if last_slice_start % seek_step:
        slice_starts = itertools.chain(slice_starts, [last_slice_start])
    for i in slice_starts:
        audio_slice = audio_segment[i:i + min_silence_len]
        if audio_slice.rms <= silence_thresh:
            silence_starts.append(i)
    if not silence_starts:
        return []
    silent_ranges = []
    prev_i = silence_starts.pop(0)
    current_range_start = prev_i
    for silence_start_i in silence_starts:
        continuous = (silence_start_i == prev_i + seek_step)
        silence_has_gap = silence_start_i > (prev_i + min_silence_len)
        if not continuous and silence_has_gap:
            silent_ranges.append([current_range_start, prev_i + min_silence_len])
            current_range_start = silence_start_i
        prev_i = silence_start_i
    silent_ranges.append([current_range_start, prev_i + min_silence_len])
    return silent_ranges


def detect_nonsilent(audio_segment, min_silence_len=1000, silence_thresh=-16, seek_step=1):
    silent_ranges = detect_silence(audio_segment, min_silence_len, silence_thresh, seek_step)
    len_seg = len(audio_segment)
    if not silent_ranges:
        return [[0, len_seg]]
    if silent_ranges[0][0] == 0 and silent_ranges[0][1] == len_seg:
        return []
    prev_end_i = 0
    nonsilent_ranges = []
    for start_i, end_i in silent_ranges:
        nonsilent_ranges.append([prev_end_i, start_i])
        prev_end_i = end_i
    if end_i != len_seg:
        nonsilent_ranges.append([prev_end_i, len_seg])
    if nonsilent_ranges[0] == [0, 0]:
        nonsilent_ranges.pop(0)
    return nonsilent_ranges


def split_ranges(audio_segment, min_silence_len=1000, silence_thresh=-16, keep_silence=100, seek_step=1):
    def pairwise(iterable):
        a, b = itertools.tee(iterable)
        next(b, None)
        return zip(a, b)

    output_ranges = [[start - keep_silence, end + keep_silence]
                     for (start, end) in detect_nonsilent(audio_segment, min_silence_len, silence_thresh, seek_step)]
    for range_i, range_ii in pairwise(output_ranges):
        last_end = range_i[1]
        next_start = range_ii[0]
        if next_start < last_end:
            range_i[1] = (last_end + next_start) // 2
            range_ii[0] = range_i[1]
    return [[max(start, 0), min(end, len(audio_segment))] for start, end in output_ranges]


def split_on_silence(audio_segment, min_silence_len=1000, silence_thresh=-16, keep_silence=100, seek_step=1):
    return [audio_segment[start:end]
            for start, end in split_ranges(audio_segment, min_silence_len, silence_thresh, keep_silence, seek_step)]


def detect_leading_silence(sound, silence_threshold=-50.0, chunk_size=10):
    trim_ms = 0
    assert chunk_size > 0
    while sound[trim_ms:trim_ms + chunk_size].dBFS < silence_threshold and trim_ms < len(sound):
        trim_ms += chunk_size
    return min(trim_ms, len(sound))


# ------------------------------------------------------------------------------------------- infer/utils_infer.py
def remove_silence_edges(audio, silence_threshold=-42):
    non_silent_start_idx = detect_leading_silence(audio, silence_threshold=silence_threshold)
    audio = audio[non_silent_start_idx:]
    non_silent_end_duration = audio.duration_seconds
    for ms in (audio[i] for i in reversed(range(len(audio)))):
        if ms.dBFS > silence_threshold:
            break
        non_silent_end_duration -= 0.001
    return audio[: int(non_silent_end_duration * 1000)]


def clip_prompt(aseg):
    """preprocess_ref_audio_text's audio half (utils_infer.py:385-417).  Returns (the segment, the rule that said "clipping short")."""
    rule = 0
    non_silent_segs = split_on_silence(aseg, min_silence_len=1000, silence_thresh=-50, keep_silence=1000, seek_step=10)
    non_silent_wave = Segment.silent(duration=0)
    for non_silent_seg in non_silent_segs:
        if len(non_silent_wave) > 6000 and len(non_silent_wave + non_silent_seg) > 12000:
            rule = 1
            break
        non_silent_wave += non_silent_seg
    if len(non_silent_wave) > 12000:
        rule = 0
        non_silent_segs = split_on_silence(aseg, min_silence_len=100, silence_thresh=-40, keep_silence=1000, seek_step=10)
        non_silent_wave = Segment.silent(duration=0)
        for non_silent_seg in non_silent_segs:
            if len(non_silent_wave) > 6000 and len(non_silent_wave + non_silent_seg) > 12000:
                rule = 2
                break
            non_silent_wave += non_silent_seg
    aseg = non_silent_wave
    if len(aseg) > 12000:
        aseg = aseg[:12000]
        rule = 3
    aseg = remove_silence_edges(aseg) + Segment.silent(duration=50)
    return aseg, rule


def remove_silence_for_generated_wav(aseg):
    non_silent_segs = split_on_silence(aseg, min_silence_len=1000, silence_thresh=-50, keep_silence=500, seek_step=10)
    non_silent_wave = Segment.silent(duration=0)
    for non_silent_seg in non_silent_segs:
        non_silent_wave += non_silent_seg
    return non_silent_wave


# ------------------------------------------------------------------------------------------------------- flags
def silence_flags(seg, min_silence_len, silence_thresh, seek_step):
    """detect_silence's per-slice decisions, one per slice start, in its order."""
    seg_len = len(seg)
    if seg_len < min_silence_len:
        return []
    thresh = db_to_float(silence_thresh) * seg.max_possible_amplitude
    last = seg_len - min_silence_len
    starts = list(range(0, last + 1, seek_step))
    if last % seek_step:
        starts.append(last)
    return [int(seg[i:i + min_silence_len].rms <= thresh) for i in starts]


def leading_flags(seg, silence_threshold=-42, chunk_size=10):
    """detect_leading_silence's test on every chunk."""
    return [int(seg[i:i + chunk_size].dBFS < silence_threshold) for i in range(0, len(seg), chunk_size)]


def trailing_flags(seg, silence_threshold=-42):
    """remove_silence_edges's test on every millisecond (1 = it does not stop the loop)."""
    return [int(not seg[i].dBFS > silence_threshold) for i in range(len(seg))]


def quantise(x: np.ndarray, qscale: float) -> np.ndarray:
    """The 16-bit view of f32 audio [channels, frames] (include/f5_hip.h)."""
    v = np.rint(np.nan_to_num(x.astype(np.float32) * np.float32(qscale), nan=0.0, posinf=32767.0, neginf=-32768.0))
    return np.clip(v, -32768, 32767).astype(np.int16)
