"""GPU: the handle-less waveform calls -- f5_edit_assemble, f5_wave_splice, f5_silence_analyse, f5_wave_gather -- share one
per-device workspace (CallState, csrc/internal.h): one arena that every call carves its tables from, one ring of 8 pinned slots,
one event that orders a call behind the one before it.  These tests issue the C-level calls back to back, with no host
synchronisation in between, and compare every result bit for bit with the oracles the two stages' own GPU tests use
(edit_oracle.py, silence_oracle.py): calls of different kinds interleaved on one stream while the arena is replaced by a larger
one, more consecutive calls than the ring has slots, and calls on two streams at once.  Every input is on the device and every
output is allocated before the first call, so that nothing but the calls themselves touches the stream."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import edit_oracle as EO  # noqa: E402
from gpu_util import DEV  # noqa: E402
from test_silence import build, materialise  # noqa: E402
from test_silence_gpu import oracle_flags, place  # noqa: E402
from test_speech_edit_gpu import HOP, fake_mel, same_bits, splice_inputs  # noqa: E402

from f5_tts_amd import _lib  # noqa: E402
from f5_tts_amd import edit as E  # noqa: E402
from f5_tts_amd import silence as S  # noqa: E402

NAN = float("nan")


def ptr(t):
    return C.c_void_p(t.data_ptr())


def stream_ptr(stream):
    return C.c_void_p((stream if stream is not None else torch.cuda.current_stream()).cuda_stream)


def ok(rc):
    assert rc == 0, _lib.load().f5_last_error().decode()


class Assemble:
    """One f5_edit_assemble call over `cases` (edit_oracle.PLAN_CASES entries) with rows of `row` elements: 16-byte accesses for
    row 100, element accesses for row 6."""

    def __init__(self, cases, row, seed):
        self.B, self.row, self.frames = len(cases), row, [c[0] for c in cases]
        mels = [fake_mel(T, seed=seed + T, row=row) for T in self.frames]
        maps = [EO.frame_map(*c) for c in cases]
        self.plans = [E.edit_plan(*c) for c in cases]
        self.D = [len(m) for m in maps]
        self.T_max = max(self.frames)
        store = torch.full((self.B, self.T_max, row), NAN)
        for b, m in enumerate(mels):
            store[b, :m.shape[0]] = m
        self.mel = store.to(DEV)
        self.want = EO.assemble(mels, maps)

    def new_out(self):
        return torch.full((self.B, max(self.D), self.row), NAN, device=DEV)

    def issue(self, out, stream=None):
        counts, segs = E.segment_table(self.plans)
        ok(_lib.load().f5_edit_assemble(ptr(self.mel), self.B, self.T_max * self.row, self.row, _lib.int_array(self.frames), counts, segs,
                                        _lib.int_array(self.D), ptr(out), max(self.D), stream_ptr(stream)))


class Silence:
    """f5_silence_analyse and f5_wave_gather over one set of items: specs is a list of (rate, int16 [C, F], pieces | None) -- the
    item is analysed and gathered through its pieces' segment table (None: the whole item as it lies)."""

    def __init__(self, specs, queries):
        self.queries, self.B = queries, len(specs)
        self.rates = [r for r, _, _ in specs]
        self.shapes = [q.shape for _, q, _ in specs]
        pieces = [p if p is not None else [(0, q.shape[1])] for _, q, p in specs]
        self.signals = [materialise(p, q) for (_, q, _), p in zip(specs, pieces)]        # what the oracle sees
        self.tables = [S.segment_table(p) for p in pieces]
        self.lens = [S.ms_len(sig.shape[1], r) for sig, r in zip(self.signals, self.rates)]
        self.views, self.buffer = place([q.astype(np.float32) / np.float32(32768.0) for _, q, _ in specs])
        base = min(v.data_ptr() for v in self.views)
        self.base, self.starts = C.c_void_p(base), [(v.data_ptr() - base) // 4 for v in self.views]
        nq, n = len(queries), self.B * len(queries)
        self.counts, self.offs, total = (C.c_int32 * n)(), (C.c_int64 * n)(), C.c_int64()
        self.q_arr = _lib.int_array([v for q in queries for v in q])
        ok(_lib.load().f5_silence_plan(self.B, _lib.int_array(self.lens), nq, self.q_arr, self.counts, self.offs, C.byref(total)))
        self.total = total.value
        self.out_frames = [sig.shape[1] for sig in self.signals]
        self.out_starts, run = [], 0
        for (c, _), n in zip(self.shapes, self.out_frames):
            run = (run + 3) // 4 * 4 + 1                                                    # every item one element off 16 bytes
            self.out_starts.append(run)
            run += c * n
        self.capacity = run

    def _items(self):
        return (self.base, self.B, (C.c_int64 * self.B)(*self.starts), _lib.int_array([c for c, _ in self.shapes]),
                _lib.int_array([f for _, f in self.shapes]))

    def _tables(self):
        flat = [int(v) for t in self.tables for seg in t for v in seg]
        return (C.c_int32 * self.B)(*[len(t) for t in self.tables]), (C.c_int32 * max(len(flat), 1))(*flat)

    def new_flags(self):
        return torch.full((self.total + 16,), 7, device=DEV, dtype=torch.uint8)

    def analyse(self, flags, stream=None):
        ok(_lib.load().f5_silence_analyse(*self._items(), _lib.int_array(self.rates), _lib.int_array(self.lens), 32768.0, len(self.queries),
                                          self.q_arr, *self._tables(), ptr(flags), self.total, stream_ptr(stream)))

    def check_flags(self, flags, what):
        host, nq = flags.cpu().numpy(), len(self.queries)
        assert (host[self.total:] == 7).all(), f"{what}: flags were written behind the plan's total"
        for b in range(self.B):
            want = oracle_flags(self.signals[b], self.rates[b], self.queries)
            for k in range(nq):
                got = host[self.offs[b * nq + k]:self.offs[b * nq + k] + self.counts[b * nq + k]]
                assert got.shape == want[k].shape and np.array_equal(got, want[k]), (what, b, self.queries[k])

    def new_gathered(self):
        return torch.full((self.capacity + 16,), NAN, device=DEV)

    def gather(self, out, stream=None):
        ok(_lib.load().f5_wave_gather(*self._items(), 32768.0, *self._tables(), _lib.int_array(self.out_frames),
                                      (C.c_int64 * self.B)(*self.out_starts), ptr(out), self.capacity, stream_ptr(stream)))

    def check_gathered(self, out, what):
        want = np.full(self.capacity + 16, np.nan, dtype=np.float32)
        for sig, o in zip(self.signals, self.out_starts):
            want[o:o + sig.size] = (sig.astype(np.float32) / np.float32(32768.0)).reshape(-1)
        assert np.array_equal(out.cpu().numpy().view(np.int32), want.view(np.int32)), f"{what}: the gathered items differ from the oracle's"


class Splice:
    """One f5_wave_splice call over a case of test_speech_edit_gpu.SPLICE_CASES, the originals with NaN between them."""

    def __init__(self, name):
        self.cf, self.items, gs, as_ = splice_inputs(name)
        self.B, self.W = len(self.items), max(it[0] for it in self.items) + 9
        gen = torch.full((self.B, self.W + 3), NAN)
        for b, g in enumerate(gs):
            gen[b, :len(g)] = torch.from_numpy(g)
        parts, self.starts, off = [], [], 0
        for a in as_:
            parts += [torch.full((3,), NAN), torch.from_numpy(a)]
            self.starts.append(off + 3)
            off += 3 + len(a)
        self.gen, self.originals = gen.to(DEV), torch.cat(parts).to(DEV)
        self.want = torch.from_numpy(np.stack([EO.splice_fold(g, a, it[2], HOP, self.cf, width=self.W) for g, a, it in zip(gs, as_, self.items)]))

    def new_out(self):
        return torch.full((self.B, self.W), NAN, device=DEV)

    def issue(self, out, stream=None):
        segs = [v for it in self.items for s in it[2] for v in s]
        ok(_lib.load().f5_wave_splice(ptr(self.gen), self.B, self.gen.stride(0), _lib.int_array([it[0] for it in self.items]), ptr(self.originals),
                                      (C.c_int64 * self.B)(*self.starts), _lib.int_array([it[1] for it in self.items]),
                                      _lib.int_array([len(it[2]) for it in self.items]), _lib.int_array(segs), HOP, self.cf, ptr(out),
                                      self.W, stream_ptr(stream)))


QUERIES = ((100, 10, 327, 0), (10, 10, 260, 1), (1, 1, 260, 1), (300, 7, 103, 0))
TWO_RECORDINGS = [EO.PLAN_CASES["fix_duration_longer"], EO.PLAN_CASES["no_parts"]]            # 3 segments and 1


def small_items():
    """Three items of 0.3 to 1.2 s at 16 and 24 kHz; the last one is read through a table with a reordered piece, a gap of silence
    and a piece that runs past the item's end."""
    a = build(24000, 1, [(100, "q"), (350, "S"), (250, "0")], seed=61)
    b = build(16000, 2, [(120, "S"), (180, "q")], seed=62)
    c = build(16000, 1, [(300, "S"), (500, "q"), (400, "S")], seed=63)
    pieces = [(3000, 4000), (100, 2000), (-1, 160), (c.shape[1] - 40, 100), (9000, 6000)]
    return [(24000, a, None), (16000, b, None), (16000, c, pieces)]


def test_interleaved_calls_on_one_stream_while_the_arena_grows():
    """Assembly (16-byte and element accesses), analysis, gather, splice, an analysis of ten times the milliseconds and the two
    assemblies again, back to back.  The larger analysis replaces the arena when nothing larger ran in this process before it (this
    file alone, or first); behind an earlier, larger call it is the interleaving alone that is checked."""
    plans = [E.edit_plan(*c) for c in TWO_RECORDINGS]
    assert [len(p[0]) for p in plans] == [3, 1]
    vec, elem = Assemble(TWO_RECORDINGS, 100, seed=70), Assemble(TWO_RECORDINGS, 6, seed=71)
    small = Silence(small_items(), QUERIES)
    assert all(300 <= n <= 1200 for n in small.lens) and len(small.tables[2]) == 4
    large = Silence([(24000, build(24000, 2, [(2500, "S"), (1500, "q"), (3000, "S"), (1200, "0"), (1800, "S")], seed=64), None),
                     (16000, build(16000, 1, [(4000, "q"), (5000, "S"), (3000, "q")], seed=65), None)], QUERIES[:2] + ((1000, 10, 103, 0),))
    assert sum(large.lens) >= 9 * sum(small.lens)
    splice = Splice("three_items")
    first = [vec.new_out(), elem.new_out()]
    again = [vec.new_out(), elem.new_out()]
    flags, gathered, spliced, flags2 = small.new_flags(), small.new_gathered(), splice.new_out(), large.new_flags()
    torch.cuda.synchronize()
    vec.issue(first[0])
    elem.issue(first[1])
    small.analyse(flags)
    small.gather(gathered)
    splice.issue(spliced)
    large.analyse(flags2)                                             # ten times the slots: the arena is replaced
    vec.issue(again[0])
    elem.issue(again[1])
    torch.cuda.synchronize()
    for call, a, b in zip((vec, elem), first, again):
        same_bits(a, call.want, f"assembly, rows of {call.row}")
        same_bits(b, a, f"assembly, rows of {call.row}, issued again behind the larger analysis")
    small.check_flags(flags, "the small analysis")
    small.check_gathered(gathered, "the gather")
    same_bits(spliced, splice.want, "the splice")
    large.check_flags(flags2, "the large analysis")


def test_more_consecutive_calls_than_the_ring_has_slots():
    calls = [Assemble([(40 + 3 * k, [(0.05 + 0.01 * k, 0.15 + 0.02 * k)], [0.02 * (k + 1)])], 100 if k % 2 == 0 else 6, seed=80 + k)
             for k in range(12)]
    assert len({tuple(c.plans[0][0]) for c in calls}) == 12           # twelve different tables
    outs = [c.new_out() for c in calls]
    torch.cuda.synchronize()
    for c, out in zip(calls, outs):
        c.issue(out)
    torch.cuda.synchronize()
    for k, (c, out) in enumerate(zip(calls, outs)):
        same_bits(out, c.want, f"call {k} of 12")


def test_calls_on_two_streams_share_the_workspace():
    """A long analysis on one stream and, at once, an assembly and a gather on another, whose tables land at the start of the
    arena the analysis works in: the results equal those of the same calls made alone.  This can catch a missing enter / leave
    around a call (the second stream's tables would overwrite prefix sums that the first stream's kernels still read); passing does
    not prove the ordering, which depends on how the two streams happen to run.  The proof is the code: every call waits for the
    event the call before it recorded behind its last kernel, under the mutex that both hold from the lookup to the record."""
    rng = np.random.default_rng(90)
    specs = []
    for k in range(16):                                               # 16 items of 20 s at 24 kHz: bursts and pauses
        q = (rng.standard_normal((1, 480000)) * 900).astype(np.int16)
        for a in range(k % 3, 20, 3):
            q[0, a * 24000:(a + 1) * 24000] //= 64
        specs.append((24000, q, None))
    long = Silence(specs, ((1000, 10, 103, 0), (100, 10, 327, 0)))
    one = Assemble([EO.PLAN_CASES["two_parts_fixed"]], 100, seed=91)
    small = Silence(small_items()[2:], QUERIES[:1])
    alone = [long.new_flags(), one.new_out(), small.new_gathered()]
    both = [long.new_flags(), one.new_out(), small.new_gathered()]
    torch.cuda.synchronize()
    long.analyse(alone[0])
    torch.cuda.synchronize()
    one.issue(alone[1])
    torch.cuda.synchronize()
    small.gather(alone[2])
    torch.cuda.synchronize()
    sa, sb = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    long.analyse(both[0], sa)
    one.issue(both[1], sb)
    small.gather(both[2], sb)
    sa.synchronize()
    sb.synchronize()
    assert 0 < int(alone[0][:long.total].sum()) < long.total           # silent and sounding windows both
    assert torch.equal(both[0], alone[0]), "the analysis differs from the analysis alone"
    same_bits(both[1], alone[1], "the assembly on the second stream")
    same_bits(alone[1], one.want, "the assembly alone")
    assert torch.equal(both[2].view(torch.int32), alone[2].view(torch.int32)), "the gather on the second stream differs from the gather alone"
    small.check_gathered(alone[2], "the gather alone")
