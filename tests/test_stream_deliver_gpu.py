"""GPU: f5_wave_deliver against the numpy fold of its contract (deliver_oracle) bit for bit -- every tested rate, the lengths at
which the window logic changes, both formats, into gpu_util.Guarded buffers from inputs that lie between NaN --, its split
invariance over final and growing streams, a mixed batch against each item alone, the quantiser table; and infer.open_stream:
the packets of a request against the pieces synthesize_script makes of its chunks, against the oracle applied to wave_join of
those pieces (cross-fade, 16 kHz, s16), batched against chunk by chunk under masked attention, and the session's state."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import DEV, Guarded  # noqa: E402

import deliver_oracle as O  # noqa: E402
from test_long_form_gpu import cached, tiny_model, tiny_vocoder  # noqa: E402

import f5_tts_amd as P  # noqa: E402
from f5_tts_amd import _lib  # noqa: E402
from f5_tts_amd import infer as I  # noqa: E402

RATES = (24000, 16000, 8000, 22050, 44100, 48000)
FORMATS = {"f32": (0, torch.float32, np.int32), "s16": (1, torch.int16, np.int16)}
EXTRA = 9


def mel_spec(rate):
    """One MelSpec for the kernel tests, with the bank of `rate` in its handle."""
    ms = cached("deliver mel", lambda: P.mel.MelSpec().to(DEV))
    I.wave_deliver(ms, [torch.zeros(1, device=DEV)], out_rate=rate)          # (uploads the bank on its first use)
    return ms, ms._handle(torch.device(DEV))


def lengths(rate):
    orig, new, width, _ = O.geometry(rate)
    return sorted({n for n in (1, 2, width, width + orig - 1, width + orig, 3 * orig + 1, 4097) if n >= 1})


def signal(n, seed):
    return (np.random.default_rng(seed).standard_normal(n) * 0.3).astype(np.float32)


def place(signals):
    """The signals as views of one device buffer with NaN in front of, between and behind them."""
    at, spans = 3, []
    for x in signals:
        spans.append(at)
        at += len(x) + 1 + len(spans) % 3
    host = torch.full((at + 2,), float("nan"))
    for a, x in zip(spans, signals):
        host[a:a + len(x)] = torch.from_numpy(x)
    dev = host.to(DEV)
    return [dev[a:a + len(x)] for a, x in zip(spans, signals)]


def deliver_call(h, views, finals, ranges, rate, fmt, out, shift=0, cap=None):
    """f5_wave_deliver into the Guarded `out`, `shift` elements in; returns (code, the items' element offsets)."""
    B = len(views)
    first = min(v.data_ptr() for v in views)
    at = (C.c_int64 * B)()
    rc = _lib.load().f5_wave_deliver(h, C.c_void_p(first), B, (C.c_int64 * B)(*[(v.data_ptr() - first) // 4 for v in views]),
                                     _lib.int_array([v.shape[0] for v in views]), _lib.int_array([int(f) for f in finals]),
                                     (C.c_int64 * B)(*[r[0] for r in ranges]), (C.c_int64 * B)(*[r[1] for r in ranges]), rate,
                                     FORMATS[fmt][0], C.c_void_p(out.ptr() + shift * out.raw.element_size()),
                                     out.n - shift if cap is None else cap, at, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    return rc, list(at)


def check_written(out, spans, wants, fmt, what):
    """spans: (first element, count) per item inside out; everything else of out must still hold the sentinel."""
    assert out.guards_intact(), f"{what}: a guard band was overwritten"
    bits = out.bits.cpu().numpy()
    mask = np.ones(out.n, bool)
    for (a, count), want in zip(spans, wants):
        assert count == len(want), (what, count, len(want))
        got = bits[a:a + count]
        ref = want.view(FORMATS[fmt][2])
        assert np.array_equal(got, ref), f"{what}: {int((got != ref).sum())} of {count} samples differ from the oracle (first at {int(np.argmax(got != ref))})"
        mask[a:a + count] = False
    assert (bits[mask] == out.sent).all(), f"{what}: an element outside the ranges was written"


@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("rate", RATES)
def test_deliver_equals_the_oracle_bit_for_bit(rate, fmt):
    ms, h = mel_spec(rate)
    for n in lengths(rate):
        x = signal(n, seed=n + rate)
        (view,) = place([x])
        for final in (True, False):
            ln, ready = O.plan(rate, n, final)
            assert I.deliver_plan(rate, n, final) == (ln, ready)
            want = O.deliver(x, rate, fmt, final)
            assert len(want) == ready
            shifts = (0, 1) if n == 4097 else (0,)                          # the output on a 16-byte multiple, and one element off it
            for shift in shifts:
                out = Guarded((shift + ready + EXTRA,), FORMATS[fmt][1])
                rc, at = deliver_call(h, [view], [final], [(0, ready)], rate, fmt, out, shift)
                torch.cuda.synchronize()
                assert rc == 0 and at == [0], _lib.load().f5_last_error().decode()
                check_written(out, [(shift, ready)], [want], fmt, f"{rate} Hz {fmt}, n = {n}, final = {final}, shift {shift}")
    # the Python wrapper: the same bits, one tensor per item
    x = signal(4097, seed=1)
    got = I.wave_deliver(ms, place([x]), out_rate=rate, sample_format=fmt)[0]
    assert got.dtype == FORMATS[fmt][1] and np.array_equal(got.cpu().numpy(), O.deliver(x, rate, fmt))


def partition(lo, hi, rng, parts):
    """[lo, hi) cut at random places, with a few one-sample ranges among the pieces."""
    if hi <= lo:
        return []
    cuts = set(rng.integers(lo, hi + 1, size=parts).tolist())
    for c in rng.integers(lo, hi, size=3).tolist():
        cuts |= {c, min(c + 1, hi)}
    edges = sorted(cuts | {lo, hi})
    return list(zip(edges[:-1], edges[1:]))


@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("rate", (16000, 22050, 48000, 24000))
def test_split_invariance_over_final_and_growing_streams(rate, fmt):
    ms, _ = mel_spec(rate)
    orig, new, width, _ = O.geometry(rate)
    n = 3001
    x = signal(n, seed=rate)
    (view,) = place([x])
    whole = I.wave_deliver(ms, [view], out_rate=rate, sample_format=fmt)[0]
    assert np.array_equal(whole.cpu().numpy(), O.deliver(x, rate, fmt))
    rng = np.random.default_rng(rate + len(fmt))
    # a finished stream in random ranges: one launch, every range an item over the same samples
    ranges = partition(0, whole.shape[0], rng, 12)
    assert any(b - a == 1 for a, b in ranges) and (new == 1 or any(a % new for a, _ in ranges)), "no one-sample range or no start inside a frame"
    parts = I.wave_deliver(ms, [view] * len(ranges), out_rate=rate, sample_format=fmt, ranges=ranges)
    assert torch.equal(torch.cat(parts), whole), "a finished stream delivered in ranges differs from one call"
    # a growing stream: what has become settled since the last visit, itself cut at random places
    sent, got = 0, []
    for seen in sorted({1, max(width + orig - 1, 1), width + orig, 700, 701, 2048, n - 1, n}):
        final = seen == n
        ready = I.deliver_plan(rate, seen, final)[1]
        assert ready >= sent
        ranges = partition(sent, ready, rng, 4)
        if ranges:
            got += I.wave_deliver(ms, [view[:seen]] * len(ranges), out_rate=rate, sample_format=fmt, ranges=ranges, final=final)
        sent = ready
    assert sent == whole.shape[0] and torch.equal(torch.cat(got), whole), "a stream delivered as it grew differs from one call"


@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("rate", (16000, 44100))
def test_a_mixed_batch_equals_each_item_alone_and_leaves_the_gaps(rate, fmt):
    ms, h = mel_spec(rate)
    orig, new, width, _ = O.geometry(rate)
    ns = [4097, 1, width + orig, 2500, 333]
    finals = [True, True, False, False, True]
    xs = [signal(n, seed=7 + i) for i, n in enumerate(ns)]
    views = place(xs)
    ready = [O.plan(rate, n, f)[1] for n, f in zip(ns, finals)]
    # whole, whole, whole, a range that starts and ends inside frames, an empty range
    ranges = [(0, ready[0]), (0, ready[1]), (0, ready[2]), (new + 1, ready[3] - 3), (5, 5)]
    wants = [O.deliver(x, rate, fmt, f, *r) for x, f, r in zip(xs, finals, ranges)]
    per16 = 4 if fmt == "f32" else 8
    spans, run = [], 0
    for a, b in ranges:
        run = (run + per16 - 1) // per16 * per16
        spans.append((run, b - a))
        run += b - a
    assert any(spans[i - 1][0] + spans[i - 1][1] < spans[i][0] for i in range(1, len(spans))), "no gap between items: the case lost its point"
    out = Guarded((run + EXTRA,), FORMATS[fmt][1])
    rc, at = deliver_call(h, views, finals, ranges, rate, fmt, out, cap=run)
    torch.cuda.synchronize()
    assert rc == 0 and at == [a for a, _ in spans], _lib.load().f5_last_error().decode()
    check_written(out, spans, wants, fmt, f"mixed batch at {rate} Hz {fmt}")
    for i in range(len(ns)):
        if ranges[i][1] > ranges[i][0]:
            alone = I.wave_deliver(ms, [views[i]], out_rate=rate, sample_format=fmt, ranges=[ranges[i]], final=finals[i])[0]
            assert np.array_equal(alone.cpu().numpy(), wants[i]), f"item {i} alone"


def test_the_quantiser_table():
    ms, _ = mel_spec(24000)
    s = np.float32(32767.0)
    x = np.array([0.5, -0.5, 1.5, 2.5], np.float32) / s
    x = np.concatenate([x, np.array([1.0, -1.0, 2.0, -2.0, np.inf, -np.inf, np.nan], np.float32)])
    want = [0, 0, 2, 2, 32767, -32767, 32767, -32768, 32767, -32768, 0]
    assert O.quantise(x).tolist() == want
    got = I.wave_deliver(ms, [torch.from_numpy(x).to(DEV)], out_rate=24000, sample_format="s16")[0]
    assert got.cpu().tolist() == want
    same = I.wave_deliver(ms, [torch.from_numpy(x).to(DEV)], out_rate=24000, sample_format="f32")[0]
    assert np.array_equal(same.cpu().numpy().view(np.int32), x.view(np.int32)), "24 kHz f32 is not a pass-through"


# ------------------------------------------------------------------------------------------------ the session
KW = dict(nfe_step=2, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=3)
SPEED = 8.0
REF_TEXT = "Oh, hello."                                      # 10 bytes over 1 s: max_chars 240, few 120, min 60


def sentence(n, c):
    return c * (n - 1) + "."


# at 240: "a b c" (55 + 1 + 55 + 1 + 117 = 229; the 12 of SHORT do not fit), SHORT, d.  First package: "a b" / c at 120, a / b at 60.
SHORT = "Hi there ok."
CHUNKS = [sentence(55, "a"), sentence(55, "b"), sentence(117, "c"), SHORT, sentence(235, "d")]
TEXT = " ".join(CHUNKS)
FADE = 3600


def voice():
    """1 s of 24 kHz mono noise, RMS 0.05 < target_rms: the rescale runs."""
    return {"main": dict(ref_audio=(torch.randn(1, 24000, generator=torch.Generator().manual_seed(5)) * 0.05, 24000), ref_text=REF_TEXT)}


def bank_of(model, masked):
    return cached(("stream bank", masked), lambda: I.prepare_voices(model, voice()))


def pieces_of(model, voc, masked):
    """Every chunk as synthesize_script speaks it alone with the bank's voice (computed once, shared, left unchanged)."""
    def make():
        bank = bank_of(model, masked)
        return [I.synthesize_script(model, voc, bank, chunk, speed=SPEED, **KW)[0] for chunk in CHUNKS]
    return cached(("stream pieces", masked), make)


def collect(session, text):
    """(packets, the session's groups_emitted at each packet)."""
    packets, groups = [], []
    for packet, rate in session.stream(text):
        assert rate == session.out_rate and isinstance(packet, np.ndarray)
        packets.append(packet)
        groups.append(session.stats()["groups_emitted"])
    return packets, groups


def test_the_plan_of_the_test_text():
    assert I.stream_limits(REF_TEXT, 1.0) == (240, 120, 60)
    assert I.stream_chunks(TEXT, REF_TEXT, 1.0, True) == CHUNKS
    assert I.stream_chunks(TEXT, REF_TEXT, 1.0, False) == [" ".join(CHUNKS[:3]), SHORT, CHUNKS[4]]


def test_stream_equals_the_chunks_of_synthesize_script_and_the_references_packets():
    model, voc = tiny_model(False), tiny_vocoder()
    pieces = pieces_of(model, voc, False)
    assert pieces[3].shape[0] == 11 * 256, "the short chunk is int(93 / 11 * 12 / 8) = 12 frames, which decode to (12 - 1) * 256 samples"
    s = I.open_stream(model, voc, (bank_of(model, False), "main"), speed=SPEED, **KW)
    packets, _ = collect(s, TEXT)
    assert all(p.dtype == np.float32 for p in packets)
    want = torch.cat(pieces).cpu().numpy()
    got = np.concatenate(packets)
    assert got.shape == want.shape and np.array_equal(got.view(np.int32), want.view(np.int32))
    # the reference slices every chunk's waveform on its own: full packets, then a short one
    assert [len(p) for p in packets] == [n for piece in pieces for n in I.packet_sizes(piece.shape[0], 2048)]
    assert s.stats() == dict(prompt_passes=0, groups_enqueued=5, groups_emitted=5, packets=len(packets))


@pytest.mark.parametrize("lookahead", [0, 1])
def test_stream_with_a_cross_fade_at_16_khz_s16_equals_the_oracle(lookahead):
    model, voc = tiny_model(False), tiny_vocoder()
    pieces = pieces_of(model, voc, False)
    assert pieces[3].shape[0] < FADE < pieces[2].shape[0], "the short chunk must be shorter than the fade"
    joined = I.wave_join(pieces, [0] + [FADE] * 4)
    offs, ns, total = I.join_plan([p.shape[0] for p in pieces], [0] + [FADE] * 4)
    assert ns[3] == pieces[3].shape[0] and offs[4] < offs[3], "no three-way overlap: the case lost its point"
    want = O.deliver(joined.cpu().numpy(), 16000, "s16")
    s = I.open_stream(model, voc, (bank_of(model, False), "main"), out_rate=16000, sample_format="s16", cross_fade_duration=0.15,
                      chunk_size=1000, lookahead=lookahead, speed=SPEED, **KW)
    packets, groups = collect(s, TEXT)
    got = np.concatenate(packets)
    assert got.dtype == np.int16 and got.shape == want.shape and np.array_equal(got, want)
    assert np.array_equal(got, I.deliver_waves(model, [joined], None, out_rate=16000, sample_format="s16")[0].cpu().numpy())
    assert sorted(set(groups)) == [1, 2, 3, 5], "the group of the short chunk settles nothing new: its emission is empty"
    for g in set(groups):                                    # every emission: full packets, then one short one
        sizes = [len(p) for p, at in zip(packets, groups) if at == g]
        assert all(n == 1000 for n in sizes[:-1]) and 1 <= sizes[-1] <= 1000
    assert s.stats()["groups_emitted"] == 5


def test_batched_equals_chunk_by_chunk_under_masked_attention():
    model, voc = tiny_model(True), tiny_vocoder()
    bank = bank_of(model, True)
    kw = dict(out_rate=22050, sample_format="s16", cross_fade_duration=0.15, speed=SPEED, **KW)
    single = I.open_stream(model, voc, (bank, "main"), **kw)
    want = np.concatenate(collect(single, TEXT)[0])
    single.reset()
    ends = single.plan(TEXT)["ends"]                         # the five chunks of a first package
    batch_frames = 3 * max(ends[1:4])                        # chunks 1 to 3 fill a group, the long one runs alone
    batched = I.open_stream(model, voc, (bank, "main"), batch_frames=batch_frames, **kw)
    assert [list(g) for g in batched.plan(TEXT)["groups"]] == [[0], [1, 2, 3], [4]]
    batched.reset()
    got = np.concatenate(collect(batched, TEXT)[0])
    assert got.shape == want.shape and np.array_equal(got, want)
    assert batched.stats()["groups_enqueued"] == 3


def test_session_state():
    model, voc = tiny_model(False), tiny_vocoder()
    calls = []
    real = model.mel_spec.prepare_ragged
    model.mel_spec.prepare_ragged = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        s = I.open_stream(model, voc, voice(), speed=SPEED, lookahead=1, **KW)
        first, _ = collect(s, TEXT)
        second, _ = collect(s, TEXT)                         # the same client again: three chunks, not five
    finally:
        del model.mel_spec.prepare_ragged
    assert calls == [1] and s.stats()["prompt_passes"] == 1 and s.stats()["groups_enqueued"] == 8
    assert np.array_equal(np.concatenate(first), torch.cat(pieces_of(model, voc, False)).cpu().numpy()), "a dict voice differs from the bank's"
    assert len(np.concatenate(second)) != len(np.concatenate(first))
    # the look-ahead counters at the first packet of each group
    for lookahead in (0, 1):
        s = I.open_stream(model, voc, (bank_of(model, False), "main"), speed=SPEED, lookahead=lookahead, **KW)
        seen = {}
        for _packet, _rate in s.stream(TEXT):
            st = s.stats()
            seen.setdefault(st["groups_emitted"], st["groups_enqueued"])
        assert seen == {g: min(g + lookahead, 5) for g in range(1, 6)}, (lookahead, seen)
    # an early close leaves the session usable: the next request equals that of a session that heard the first one out
    a = I.open_stream(model, voc, (bank_of(model, False), "main"), out_rate=16000, speed=SPEED, lookahead=1, **KW)
    gen = a.stream(TEXT)
    next(gen)
    gen.close()
    after_close = np.concatenate(collect(a, TEXT)[0])
    b = I.open_stream(model, voc, (bank_of(model, False), "main"), out_rate=16000, speed=SPEED, lookahead=1, **KW)
    collect(b, TEXT)
    fresh = np.concatenate(collect(b, TEXT)[0])
    assert np.array_equal(after_close.view(np.int32), fresh.view(np.int32))
    a.reset()
    assert len(a.plan(TEXT)["chunks"]) == 5
