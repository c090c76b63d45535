"""CPU: the host arithmetic of silence clipping (silence.py) against the literal restatement of pydub and the reference drivers in
silence_oracle.py, given the oracle's own per-slice decisions as flags; the integer threshold rule of include/f5_hip.h against
audioop.rms; the 50 ms tail against audioop.ratecv; and the argument checks of the three C entry points (no GPU, nothing launched).

The plans only ever see flags and lengths; the audio is touched by the oracle alone, and by `materialise`, which copies the frames
a plan names."""
import ctypes as C
import math

import numpy as np
import pytest

import silence_oracle as O
from silence_oracle import audioop

from f5_tts_amd import _lib
from f5_tts_amd import silence as S

LOUD, QUIET = 3000, 20      # peak of the "speech" (rms ~1700, above every threshold) and of the "room" (rms ~12, below every one)


def build(rate, channels, parts, seed=0):
    """int16 [channels, frames]: parts is a list of (ms, 'S' speech | 'q' quiet room noise | '0' digital silence)."""
    rng = np.random.default_rng(seed)
    out = []
    for ms, kind in parts:
        n = int(rate * ms / 1000)
        amp = {"S": LOUD, "q": QUIET, "0": 0}[kind]
        out.append(rng.integers(-amp, amp + 1, size=(channels, n)).astype(np.int16))
    return np.concatenate(out, axis=1)


CASES = {
    "long_pauses_rule1": [(4000, "S"), (1500, "q"), (4000, "S"), (1500, "0"), (5000, "S")],
    "short_pauses_rule2": [(1400, "S"), (300, "q")] * 3 + [(1400, "S"), (900, "q")] + [(1400, "S"), (100, "0")] * 3 + [(1400, "S")],
    "no_pause_rule3": [(13000, "S")],
    "three_seconds_edges_only": [(215, "q"), (2600, "S"), (187, "0")],
    "all_silent": [(2000, "q")],
    "shorter_than_the_window": [(700, "S")],
    "last_start_off_the_step": [(900, "S"), (1105, "q"), (340, "S")],
    "overlapping_keep_silence": [(2000, "S"), (1300, "q"), (2000, "S"), (1990, "q")],
    "one_frame": None,
}
LAYOUTS = [(24000, 1), (44100, 2), (11025, 1), (11025, 2)]


def case_audio(name, rate, channels):
    if name == "one_frame":
        return np.full((channels, 1), 1234, dtype=np.int16)
    return build(rate, channels, CASES[name], seed=len(name) + rate + channels)


def materialise(pieces, q):
    """The frames a piece list names: [channels, frames]; silence pieces and frames at or past the item's end are zeros."""
    out = np.zeros((q.shape[0], S.signal_frames(pieces)), dtype=np.int16)
    at = 0
    for src, n in pieces:
        if src >= 0:
            have = max(min(src + n, q.shape[1]) - src, 0)
            out[:, at:at + have] = q[:, src:src + have]
        at += n
    return out


def plan_clip(q, rate):
    """silence.py's prompt pipeline, every flag taken from the oracle's own decisions on the signal in question."""
    seg = O.Segment.from_array(q, rate)
    pieces, rule = S.prompt_clip_plan(O.silence_flags(seg, 1000, -50, 10), O.silence_flags(seg, 100, -40, 10), q.shape[1], rate)
    sig = O.Segment.from_array(materialise(pieces, q), rate)
    assert len(sig) == S.ms_len(S.signal_frames(pieces), rate)
    lead = S.leading_trim(O.leading_flags(sig), len(sig))
    rest, same_grid = S.after_lead(pieces, rate, lead)
    rseg = O.Segment.from_array(materialise(rest, q), rate)
    own = O.trailing_flags(rseg)
    if same_grid:   # the claim clip_prompts relies on: the signal's per-millisecond flags serve the part behind the lead
        assert O.trailing_flags(sig)[lead:] == own
    keep = S.trailing_cut(own, S.signal_frames(rest), rate)
    final, frames = S.finish_prompt(rest, keep, rate)
    assert frames == S.signal_frames(final)
    return materialise(final, q), rule, same_grid


@pytest.mark.parametrize("rate,channels", LAYOUTS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_prompt_clip_plan_against_the_oracle(name, rate, channels):
    q = case_audio(name, rate, channels)
    want, want_rule = O.clip_prompt(O.Segment.from_array(q, rate))
    got, rule, _ = plan_clip(q, rate)
    assert rule == want_rule
    if name == "all_silent":   # nothing but silence: the reference is left with its 11025 Hz mono placeholder and the 50 ms tail
        assert (want.rate, want.channels, want.frame_count()) == (11025, 1, 551) and not want.array().any()
        want = O.Segment.silent(50).set_frame_rate(rate).set_channels(channels)
    assert want.rate == rate and want.channels == channels
    assert got.shape == want.array().shape
    assert np.array_equal(got, want.array())


def test_the_cases_reach_the_rules_they_are_named_for():
    rules = {name: O.clip_prompt(O.Segment.from_array(case_audio(name, 24000, 1), 24000))[1] for name in CASES}
    assert rules["long_pauses_rule1"] == 1 and rules["short_pauses_rule2"] == 2 and rules["no_pause_rule3"] == 3
    assert rules["three_seconds_edges_only"] == 0
    for name in ("long_pauses_rule1", "short_pauses_rule2", "no_pause_rule3"):
        seg = O.clip_prompt(O.Segment.from_array(case_audio(name, 24000, 1), 24000))[0]
        assert 6000 < len(seg) <= 12050
    # 11025 Hz with 210 ms of leading silence: the part behind the lead is on a grid of its own
    assert plan_clip(case_audio("three_seconds_edges_only", 11025, 1), 11025)[2] is False
    assert plan_clip(case_audio("three_seconds_edges_only", 24000, 1), 24000)[2] is True


@pytest.mark.parametrize("rate,channels", LAYOUTS)
@pytest.mark.parametrize("name", ["long_pauses_rule1", "all_silent", "shorter_than_the_window", "last_start_off_the_step",
                                  "overlapping_keep_silence"])
def test_ranges_and_remove_silence_plan_against_the_oracle(name, rate, channels):
    q = case_audio(name, rate, channels)
    seg = O.Segment.from_array(q, rate)
    L = len(seg)
    assert L == S.ms_len(q.shape[1], rate)
    for W, s, db, keep in ((1000, 10, -50, 1000), (100, 10, -40, 1000), (1000, 10, -50, 500), (300, 7, -50, 100)):
        flags = O.silence_flags(seg, W, db, s)
        assert len(flags) == len(S.query_starts(L, W, s))
        silent = S.silent_ranges(flags, L, W, s)
        assert silent == O.detect_silence(seg, W, db, s)
        assert S.nonsilent_ranges(silent, L) == O.detect_nonsilent(seg, W, db, s)
        assert S.split_on_silence(flags, L, W, s, keep) == O.split_ranges(seg, W, db, keep, s)
    want = O.remove_silence_for_generated_wav(seg)
    got = materialise(S.remove_silence_plan(O.silence_flags(seg, 1000, -50, 10), q.shape[1], rate), q)
    if want.frame_count() == 0:
        assert name == "all_silent" and got.shape[1] == 0
    else:
        assert np.array_equal(got, want.array())


def test_query_grid_details():
    assert S.query_starts(999, 1000, 10) == []                                  # L < W
    assert S.query_starts(1000, 1000, 10) == [0]
    assert S.query_starts(1025, 1000, 10) == [0, 10, 20, 25]                    # (L - W) % s != 0: the extra start
    assert S.query_starts(25, 10, 10, S.KIND_CHUNKS) == [0, 10, 20]
    assert S.nonsilent_ranges([], 50) == [[0, 50]] and S.nonsilent_ranges([[0, 50]], 50) == []
    assert S.nonsilent_ranges([[0, 20]], 50) == [[20, 50]]                      # the leading [0, 0] is dropped
    assert S.nonsilent_ranges([[10, 50]], 50) == [[0, 10]]                      # no final range when the silence ends at L
    assert S.split_ranges([[0, 100], [300, 400]], 400, 150) == [[0, 200], [200, 400]]


# ------------------------------------------------------------------------------------------------- the integer rule
def four_squares(t):
    for a in range(math.isqrt(t), -1, -1):
        r1 = t - a * a
        for b in range(math.isqrt(r1), -1, -1):
            r2 = r1 - b * b
            for c in range(math.isqrt(r2), -1, -1):
                d = math.isqrt(r2 - c * c)
                if d * d == r2 - c * c:
                    return a, b, c, d
    raise AssertionError(t)


def window_with_sum(cnt, k, delta):
    """cnt samples whose squares add up to cnt * k^2 + delta exactly."""
    w = np.full(cnt, k, dtype=np.int16)
    w[:4] = four_squares(4 * k * k + delta)
    assert int((w.astype(np.int64) ** 2).sum()) == cnt * k * k + delta
    return w


def test_integer_threshold_rule_against_audioop_rms():
    """E < cnt * (T + 1)^2  <=>  audioop.rms <= the float threshold, at the sums where the two could part."""
    T_edge = S.dbfs_threshold(-42)
    assert (S.rms_threshold(-50), S.rms_threshold(-40), T_edge) == (103, 327, 260)
    assert [q[2] for q in S.CLIP_QUERIES + S.EDGE_QUERIES + S.REMOVE_QUERIES] == [103, 327, 260, 260, 103]
    rng = np.random.default_rng(5)
    checked = 0
    for cnt in (24, 48, 441, 24000, 96000, 384000):
        windows = [window_with_sum(cnt, k, d) for T in (103, 327, 260) for k in (T, T + 1) for d in (-1, 0, 1)]
        windows += [rng.integers(-a, a + 1, size=cnt).astype(np.int16) for a in (150, 180, 400, 460, 570, 32767)]
        windows += [np.zeros(cnt, dtype=np.int16), np.full(cnt, -32768, dtype=np.int16)]
        for w in windows:
            E = int((w.astype(np.int64) ** 2).sum())
            rms = audioop.rms(w.tobytes(), 2)
            for db in (-50, -40):
                T = S.rms_threshold(db)
                assert (E < cnt * (T + 1) ** 2) == (rms <= O.db_to_float(db) * 32768), (cnt, E, db)
            dbfs = O.ratio_to_db(rms / 32768)
            assert (E < cnt * (T_edge + 1) ** 2) == (dbfs < -42) == (not dbfs > -42), (cnt, E)
            checked += 1
    assert checked == 6 * 26


def test_tail_formula_against_ratecv():
    for rate in (11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 176400, 192000):
        seg = O.Segment.silent(50).set_frame_rate(rate)
        assert seg.frame_count() == S.silent_tail_frames(rate), rate
    assert O.Segment.silent(50).frame_count() == 551 and S.silent_tail_frames(24000) == 1198


def test_silence_module_is_pure_python():
    import os
    src = open(os.path.join(_lib.HERE, "silence.py")).read()
    assert "import torch" not in src and "import audioop" not in src and "import numpy" not in src


# ------------------------------------------------------------------------------------------------- the C entry points
def i32(vals):
    return (C.c_int32 * len(vals))(*vals)


def i64(vals):
    return (C.c_int64 * len(vals))(*vals)


def test_silence_plan_counts_and_refusals():
    lib = _lib.load()
    lens = [0, 1, 25, 999, 1000, 1025, 12345]
    queries = [(1000, 10, 103, 0), (100, 10, 327, 0), (10, 10, 260, 1), (1, 1, 260, 1), (300, 7, 103, 0)]
    B, nq = len(lens), len(queries)
    counts, starts, total = (C.c_int32 * (B * nq))(), (C.c_int64 * (B * nq))(), C.c_int64()
    q = i32([v for qq in queries for v in qq])
    assert lib.f5_silence_plan(B, i32(lens), nq, q, counts, starts, C.byref(total)) == 0
    run = 0
    for b, L in enumerate(lens):
        for k, (W, s, _T, kind) in enumerate(queries):
            assert counts[b * nq + k] == len(S.query_starts(L, W, s, kind)) and starts[b * nq + k] == run
            run += counts[b * nq + k]
    assert total.value == run

    def refused(word, B_=B, lens_=lens, nq_=nq, q_=q, counts_=counts):
        rc = lib.f5_silence_plan(B_, i32(lens_) if lens_ is not None else None, nq_, q_, counts_, starts, C.byref(total))
        assert rc == -1 and word.encode() in lib.f5_last_error(), lib.f5_last_error()

    refused("B = 0", B_=0)
    refused("B = 65536", B_=65536)
    refused("len_ms_host", lens_=None)
    refused("nq = 9", nq_=9)
    refused("nq = 0", nq_=0)
    refused("queries_host", q_=None)
    refused("count_out", counts_=None)
    refused("L = -1", lens_=[5, -1] + lens[2:])
    refused("L = 16777217", lens_=[(1 << 24) + 1] + lens[1:])
    refused("W = 0", q_=i32([0, 10, 103, 0] * nq))
    refused("s = 0", q_=i32([10, 0, 103, 0] * nq))
    refused("T = 32768", q_=i32([10, 10, 32768, 0] * nq))
    refused("kind = 2", q_=i32([10, 10, 103, 2] * nq))


def test_analyse_and_gather_refuse_bad_arguments_without_a_gpu():
    lib = _lib.load()
    fake = C.c_void_p(4096)                                  # never dereferenced: every call below is refused before any HIP call
    good = dict(B=2, start=[0, 64], ch=[1, 2], fr=[100, 24], rate=[24000, 44100], L=[4, 1], qscale=32768.0, nq=1, q=[1, 1, 260, 1],
                segc=None, segs=None, flags=fake, cap=1 << 20)

    def analyse(word, **kw):
        a = dict(good, **kw)
        arr = lambda v, f: None if v is None else f(v)       # noqa: E731
        rc = lib.f5_silence_analyse(a.get("base", fake), a["B"], arr(a["start"], i64), arr(a["ch"], i32), arr(a["fr"], i32),
                                    arr(a["rate"], i32), arr(a["L"], i32), a["qscale"], a["nq"], arr(a["q"], i32), arr(a["segc"], i32),
                                    arr(a["segs"], i32), a["flags"], a["cap"], None)
        assert rc == -1 and word.encode() in lib.f5_last_error(), lib.f5_last_error()

    analyse("null base", base=None)
    analyse("B = 0", B=0)
    analyse("B = 65536", B=65536)
    analyse("start_host", start=None)
    analyse("channels_host", ch=None)
    analyse("frames_host", fr=None)
    analyse("rate_host", rate=None)
    analyse("len_ms_host", L=None)
    analyse("null flags", flags=None)
    analyse("nq = 9", nq=9)
    analyse("qscale", qscale=0.0)
    analyse("qscale", qscale=float("nan"))
    analyse("qscale", qscale=65536.0)
    analyse("start = -1", start=[0, -1])
    analyse("channels = 0", ch=[0, 2])
    analyse("frames = 0", fr=[100, 0])
    analyse("channels * frames", ch=[1, 2], fr=[100, 1 << 30])
    analyse("rate = 11024", rate=[24000, 11024])
    analyse("rate = 384001", rate=[384001, 44100])
    analyse("L = 16777217", L=[4, (1 << 24) + 1])
    analyse("flags_capacity", cap=4)
    analyse("segs_host", segc=[1, 0], segs=None)
    analyse("0 frames", segc=[1, 0], segs=[0, 0, 0])
    analyse("source frame -1", segc=[1, 0], segs=[0, -1, 5])
    analyse("inside or before", segc=[2, 0], segs=[0, 0, 5, 4, 9, 5])
    analyse("-1 segments", segc=[-1, 0], segs=[0, 0, 1])

    ggood = dict(B=2, start=[0, 64], ch=[1, 2], fr=[100, 24], qscale=32767.0, segc=[1, 1], segs=[0, 0, 10, 2, 5, 4], outf=[10, 6],
                 outs=[0, 12], out=fake, cap=24)

    def gather(word, **kw):
        a = dict(ggood, **kw)
        arr = lambda v, f: None if v is None else f(v)       # noqa: E731
        rc = lib.f5_wave_gather(a.get("base", fake), a["B"], arr(a["start"], i64), arr(a["ch"], i32), arr(a["fr"], i32), a["qscale"],
                                arr(a["segc"], i32), arr(a["segs"], i32), arr(a["outf"], i32), arr(a["outs"], i64), a["out"], a["cap"],
                                None)
        assert rc == -1 and word.encode() in lib.f5_last_error(), lib.f5_last_error()

    gather("null base", base=None)
    gather("B = 0", B=0)
    gather("start_host", start=None)
    gather("channels_host", ch=None)
    gather("frames_host", fr=None)
    gather("seg_count_host", segc=None)
    gather("segs_host", segs=None)
    gather("out_frames_host", outf=None)
    gather("out_start_host", outs=None)
    gather("null out", out=None)
    gather("qscale", qscale=-1.0)
    gather("out_frames = -1", outf=[10, -1])
    gather("frames = 0", fr=[0, 24])
    gather("the limit is 6", segs=[0, 0, 10, 3, 5, 4])       # item 1's segment ends at frame 7 of 6
    gather("inside or before", segc=[2, 0], segs=[0, 0, 5, 4, 9, 5])
    gather("out_capacity", cap=23)
    gather("out_capacity", outs=[-4, 12])


# ------------------------------------------------------------------------------------------------- the switches
def test_the_switches_are_off_by_default_and_need_the_device_route():
    import inspect

    import torch

    from f5_tts_amd import infer as I

    for fn, names in ((I.prompt_batch, ["clip_silence"]), (I.synthesize_long, ["clip_silence"]),
                      (I.synthesize_prompts, ["clip_silence", "remove_silence"]),
                      (I.infer_batch_process, ["clip_silence", "remove_silence"]), (I.infer_process, ["clip_silence", "remove_silence"])):
        sig = inspect.signature(fn)
        assert all(sig.parameters[n].default is False for n in names), fn.__name__
    audio = torch.zeros(1, 24000)
    with pytest.raises(ValueError, match="prompt_on_device"):
        I.prompt_batch([(audio, 24000, "a.")], ["b."], mel_spec=None, clip_silence=True)
    with pytest.raises(ValueError, match="prompt_on_device"):
        I.infer_process((audio, 24000), "a.", "b.", None, None, show_info=None, clip_silence=True)
    with pytest.raises(ValueError, match="prompt_on_device"):
        next(I.infer_batch_process((audio, 24000), "a.", ["b."], None, None, batched=True, clip_silence=True))
    with pytest.raises(ValueError, match="batched=True"):
        next(I.infer_batch_process((audio, 24000), "a.", ["b."], None, None, remove_silence=True))
    with pytest.raises(ValueError, match="11025"):
        I._check_rates("clip_prompts", [8000], 1)
    with pytest.raises(RuntimeError, match="GPU"):
        I.clip_prompts([audio], [24000], device="cpu")
    with pytest.raises(RuntimeError, match="GPU"):
        I.remove_silence([audio[0]])
