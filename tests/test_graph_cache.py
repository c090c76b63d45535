"""CPU: the host model of the sample() graph cache (tests/graph_cache_oracle.py) on hand-written sequences whose paths and counters are
written out literally, and the Python wrapper's refusal of a capacity outside [16, 64].  tests/test_graph_cache_gpu.py holds the engine
to the same model."""
import pytest

import f5_tts_amd as P
import graph_cache_oracle as G
from graph_cache_oracle import GraphCacheModel, ItemSig, Sig


def st(captures, replays, eager, evictions):
    return dict(captures=captures, replays=replays, eager=eager, evictions=evictions)


def batch(cfg, N=48, **kw):
    """A B = 2 call with lengths: never the unconditional-embedding cache."""
    return Sig(B=2, N=N, nt=12, steps=2, cfg=cfg, lens="ragged", **kw)


def test_second_sighting_captures_and_a_capture_counts_once():
    m = GraphCacheModel()
    a, b = batch(2.0), batch(2.25)
    assert m.sample(a) == ("eager", st(0, 0, 1, 0))
    assert m.sample(b) == ("eager", st(0, 0, 2, 0))
    assert m.sample(a) == ("capture", st(1, 0, 2, 0))
    assert m.sample(a) == ("replay", st(1, 1, 2, 0))
    assert m.sample(b) == ("capture", st(2, 1, 2, 0))
    assert m.sample(batch(2.0, traj=False)) == ("eager", st(2, 1, 3, 0))          # (another signature: the trajectory is part of it)
    assert m.sample(batch(2.0, method="midpoint")) == ("eager", st(2, 1, 4, 0))
    m.reset_stats()
    assert m.sample(b) == ("replay", st(0, 1, 0, 0))


def test_eviction_is_first_in_first_out_and_the_evicted_stay_warm():
    m = GraphCacheModel()
    m.reserve(2, 48, 2)
    sigs = [batch(2.0 + 0.25 * i) for i in range(17)]
    for i, s in enumerate(sigs):
        assert m.sample(s)[0] == "eager"
        path, stats = m.sample(s)
        assert path == "capture" and stats == st(i + 1, 0, i + 1, 1 if i == 16 else 0)
    # held now: signatures 1 .. 16 (0 was pushed out by 16)
    assert m.sample(sigs[0]) == ("capture", st(18, 0, 17, 2))     # still warm: captured again, pushing out 1
    assert m.sample(sigs[2]) == ("replay", st(18, 1, 17, 2))      # resident; the replay renews nothing
    assert m.sample(sigs[1]) == ("capture", st(19, 1, 17, 3))     # pushes out 2, the oldest capture, although it has just replayed
    assert m.sample(sigs[2]) == ("capture", st(20, 1, 17, 4))     # (under LRU this would have been a replay)
    assert m.sample(sigs[16]) == ("replay", st(20, 2, 17, 4))


def test_growth_clears_and_forgets_what_was_warm():
    m = GraphCacheModel()
    a = batch(2.0)
    assert [m.sample(a)[0] for _ in range(3)] == ["eager", "capture", "replay"]
    assert m.sample(batch(2.0, N=96)) == ("eager", st(1, 1, 2, 0))              # more frames than reserved: a clear, no eviction
    assert m.sample(a) == ("eager", st(1, 1, 3, 0))                             # not warm any more
    assert m.sample(a) == ("capture", st(2, 1, 3, 0))
    assert m.sample(batch(2.0, N=96)) == ("capture", st(3, 1, 3, 0))            # fits what is reserved now: nothing was cleared
    assert m.sample(Sig(B=2, N=48, nt=40, steps=2, cfg=2.0, lens="ragged")) == ("eager", st(3, 1, 4, 0))   # a longer text
    assert m.sample(a) == ("eager", st(3, 1, 5, 0))
    assert m.sample(Sig(B=3, N=48, nt=12, steps=2, cfg=2.0, lens="ragged")) == ("eager", st(3, 1, 6, 0))   # a larger batch
    assert m.sample(a) == ("eager", st(3, 1, 7, 0))
    assert m.sample(Sig(B=2, N=48, nt=12, steps=6, cfg=2.0, lens="ragged")) == ("eager", st(3, 1, 8, 0))   # more steps
    assert m.sample(a) == ("eager", st(3, 1, 9, 0))
    assert m.sample(a) == ("capture", st(4, 1, 9, 0))
    assert m.reserve(2, 48, 6) == (None, st(4, 1, 9, 0)) and m.sample(a)[0] == "replay"      # nothing grows
    assert m.reserve(2, 97, 6) == (None, st(4, 2, 9, 0)) and m.sample(a)[0] == "eager"


def test_first_per_item_call_and_more_time_rows_clear():
    m = GraphCacheModel()
    m.reserve(2, 48, 4)
    a = batch(2.0)
    assert [m.sample(a)[0] for _ in range(3)] == ["eager", "capture", "replay"]
    it = ItemSig(B=2, N=48, nt=12, steps=2, U=2, lens="ragged")
    assert m.sample_items(it) == ("eager", st(1, 1, 2, 0))          # the first per-item call clears
    assert m.sample(a) == ("eager", st(1, 1, 3, 0))
    assert m.sample_items(it) == ("capture", st(2, 1, 3, 0))        # the second does not
    assert m.sample(a) == ("capture", st(3, 1, 3, 0))
    assert m.sample_items(ItemSig(B=2, N=48, nt=12, steps=2, U=3, lens="ragged")) == ("eager", st(3, 1, 4, 0))   # more time rows
    assert m.sample_items(it) == ("eager", st(3, 1, 5, 0))
    assert m.sample_items(ItemSig(B=2, N=48, nt=12, steps=2, U=1, lens="ragged")) == ("eager", st(3, 1, 6, 0))   # fewer: its own key
    assert m.sample_items(it) == ("capture", st(4, 1, 6, 0))


def test_unconditional_embedding_key_and_the_eager_store():
    one = lambda N: Sig(B=1, N=N, nt=12, steps=2, cfg=2.0)   # noqa: E731
    m = GraphCacheModel(uc_arch=True)
    m.reserve(1, 96, 2)
    assert m.sample(one(48)) == ("eager", st(0, 0, 1, 0))        # stores the embedding of N = 48
    assert m.sample(one(48)) == ("capture", st(1, 0, 1, 0))      # "|uc"
    assert m.sample(one(48)) == ("replay", st(1, 1, 1, 0))
    assert m.sample(one(96)) == ("eager", st(1, 1, 2, 0))        # stores N = 96
    assert m.sample(one(48)) == ("eager", st(1, 1, 3, 0))        # must store N = 48 again: eager although its graph is held
    assert m.sample(one(48)) == ("replay", st(1, 2, 3, 0))       # ... and still valid
    assert m.sample(one(96)) == ("eager", st(1, 2, 4, 0))        # alternating lengths never capture
    assert m.sample(Sig(B=1, N=96, nt=12, steps=2, cfg=0.0)) == ("eager", st(1, 2, 5, 0))     # no guidance: "|nouc", plain rules
    assert m.sample(Sig(B=1, N=96, nt=12, steps=2, cfg=0.0)) == ("capture", st(2, 2, 5, 0))
    # an architecture whose embedding depends on the text: no cache, the plain rules at every N
    p = GraphCacheModel(uc_arch=False)
    p.reserve(1, 96, 2)
    assert [p.sample(one(n))[0] for n in (48, 48, 96, 48, 96, 96)] == ["eager", "capture", "eager", "replay", "capture", "replay"]
    assert G.uc_arch(P.config.F5TTS_TINY) and G.uc_arch(P.config.F5TTS_BASE) and not G.uc_arch(P.config.F5TTS_V1_BASE)
    assert not G.uc_arch(P.config.F5TTS_TINY, "MMDiT")


def test_length_buckets_capacity_and_prepare():
    m = GraphCacheModel()
    m.reserve(2, 96, 2)
    m.set_graph_capacity(20)
    sigs = [batch(2.0 + 0.25 * i) for i in range(20)]
    for s in sigs:
        m.sample(s), m.sample(s)
    assert m.stats == st(20, 0, 20, 0)
    assert m.set_graph_capacity(16) == (None, st(20, 0, 20, 4))                 # the oldest four go at once
    assert [m.sample(s)[0] for s in sigs[:4] + sigs[8:9]] == ["capture"] * 4 + ["replay"]   # 0 .. 3 push out 4 .. 7
    assert m.stats == st(24, 1, 20, 8)
    m.set_graph_capacity(32)
    assert m.set_length_buckets(32) == (None, st(24, 1, 20, 8)) and m.capacity == 16 and not m.held and not m.warm
    # granule 32: N = 33 and N = 60 share the bucket of 64, whatever the text length; a ragged batch keeps its exact key
    eq = lambda N, nt: Sig(B=2, N=N, nt=nt, steps=2, cfg=2.0, lens="equal")   # noqa: E731
    m.reset_stats()
    assert [m.sample(eq(*a))[0] for a in ((33, 12), (60, 9), (64, 12), (65, 12))] == ["eager", "capture", "replay", "eager"]
    assert m.sample(batch(2.0, N=60)) == ("eager", st(1, 1, 3, 0))
    # prepare: 17 buckets of B = 1 raise the capacity to 17 and replay on their first call; an unprepared signature pushes out the oldest
    q = GraphCacheModel()
    q.set_length_buckets(32)
    assert q.prepare(1, 32, 17 * 32, 40, 2, 2.0) == (None, st(17, 0, 0, 0)) and q.capacity == 17
    one = lambda N, cfg=2.0: Sig(B=1, N=N, nt=12, steps=2, cfg=cfg)   # noqa: E731
    assert [q.sample(one(32 * k - 5))[0] for k in range(1, 18)] == ["replay"] * 17
    assert q.sample(one(40, 2.25)) == ("eager", st(17, 17, 1, 0))
    assert q.sample(one(40, 2.25)) == ("capture", st(18, 17, 1, 1))
    assert q.sample(one(20)) == ("capture", st(19, 17, 1, 2))       # the oldest prepared bucket went; prepared counts as seen
    assert q.sample(one(40)) == ("capture", st(20, 17, 1, 3))       # ... which pushed out the second
    assert q.prepare(1, 32, 64, 40, 2, 2.0) == (None, st(20, 17, 1, 3)) and q.capacity == 17   # held already; never lowers


def test_graphs_off_is_all_eager():
    m = GraphCacheModel(graphs=False)
    assert [m.sample(batch(2.0)) for _ in range(3)][-1] == ("eager", st(0, 0, 3, 0))


@pytest.mark.parametrize("n", [15, 65])
def test_capacity_outside_16_to_64_is_refused_at_the_wrapper(n):
    tr = P.DiT(**P.config.F5TTS_TINY, text_num_embeds=40, mel_dim=100)
    with pytest.raises(ValueError, match=str(n)):
        tr.set_graph_capacity(n)
    assert tr.graph_capacity == 0
    with pytest.raises(ValueError, match=str(n)):
        GraphCacheModel().set_graph_capacity(n)
    tr.set_graph_capacity(16), tr.set_graph_capacity(64)
    assert tr.graph_capacity == 64
