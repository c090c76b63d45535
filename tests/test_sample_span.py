"""CPU: sliced ODE solves as far as they go without a device -- pool_slice against hand-written tables, CFM.sample_span's sub-grids,
noise, `done` and refusals with a recording engine, the refusals of f5_sample_span / f5k_span_stage that are decided before the
engine or the device is looked at, and a pool with a recording model: slice_steps=None makes today's calls, slice_steps=2 the
expected sequence of sample_span calls."""
import ctypes as C

import pytest
import torch

import f5_tts_amd as P
from f5_tts_amd import _lib
from f5_tts_amd import cfm as CFM_MOD
from f5_tts_amd import infer as I
from f5_tts_amd.stream import pool_slice, pool_tick, span_prev

F5_EINVAL = -1


# ------------------------------------------------------------------------------------------------ pool_slice
def test_rows_under_way_come_first_and_waiting_chunks_join_round_robin():
    under = [(4, 1, 300), (2, 2, 500)]                                   # in the order they joined, not by id
    waiting = [(2, 3, [400, 400]), (5, 1, [200])]
    assert pool_slice(under, waiting, None, 64, True, 0) == ([(4, 1), (2, 2), (2, 3), (5, 1), (2, 4)], 0)
    # the round-robin starts at the cursor, as pool_tick's does
    assert pool_slice(under, waiting, None, 64, True, 5) == ([(4, 1), (2, 2), (5, 1), (2, 3), (2, 4)], 5)
    # with nothing under way it is pool_tick
    for cursor in (0, 3, 5, 9):
        assert pool_slice([], waiting, 1200, 64, True, cursor) == pool_tick(waiting, 1200, 64, True, cursor)


def test_the_budget_holds_with_a_long_row_under_way():
    under = [(1, 1, 1000)]
    waiting = [(2, 1, [100, 100]), (3, 2, [100])]
    # rows x longest row: 3 x 1000 fits 3000, a fourth row (request 2's second chunk) does not: the tick ends there, at request 2
    assert pool_slice(under, waiting, 3000, 64, True, 0) == ([(1, 1), (2, 1), (3, 2)], 2)
    assert pool_slice(under, waiting, 4000, 64, True, 0) == ([(1, 1), (2, 1), (3, 2), (2, 2)], 0)
    assert pool_slice(under, waiting, 2999, 64, True, 0) == ([(1, 1), (2, 1)], 3)
    assert pool_slice(under, waiting, 1999, 64, True, 0) == ([(1, 1)], 2)
    assert pool_slice(under, waiting, 10, 64, True, 0) == ([(1, 1)], 2), "the first row is always taken"
    assert pool_slice(under, waiting, None, 2, True, 0) == ([(1, 1), (2, 1)], 3), "max_items counts rows under way"
    # a row under way that does not fit keeps everything behind it out, and the cursor stays
    assert pool_slice([(1, 1, 1000), (4, 1, 1000), (5, 1, 10)], waiting, 1500, 64, True, 7) == ([(1, 1)], 7)


def test_a_first_chunk_parks_the_other_rows_and_they_resume():
    under = [(1, 2, 800), (2, 1, 800)]
    waiting = [(1, 3, [800]), (3, 0, [90, 700]), (4, 0, [120])]
    assert pool_slice(under, waiting, 4000, 64, True, 0) == ([(3, 0), (4, 0)], 0), "only first chunks, in submission order"
    # the first chunks are now under way; a later first chunk waits behind them; the long rows stay parked
    under2 = under + [(3, 0, 90), (4, 0, 120)]
    waiting2 = [(1, 3, [800]), (3, 1, [700]), (6, 0, [50])]
    assert pool_slice(under2, waiting2, 4000, 64, True, 0) == ([(3, 0), (4, 0), (6, 0)], 0)
    assert pool_slice(under2, waiting2, 300, 64, True, 0) == ([(3, 0), (4, 0)], 0), "the budget holds among first chunks too"
    # no first chunk left: the parked rows resume in the order they joined, then the round-robin
    assert pool_slice(under, [(1, 3, [800]), (3, 1, [700])], 4000, 64, True, 0) == ([(1, 2), (2, 1), (1, 3), (3, 1)], 0)
    # first_alone off: a first chunk is a waiting chunk like any other
    assert pool_slice(under, waiting, 4000, 64, False, 0) == ([(1, 2), (2, 1), (1, 3), (3, 0), (4, 0)], 3)


def test_nobody_is_passed_over_twice_in_a_row():
    """pool_tick's property, with rows under way taking part of the budget: the request a tick ended at is first in the next."""
    under = [(0, 1, 500)]
    waiting = [(1, 1, [500, 500]), (2, 1, [500, 500]), (3, 1, [500, 500])]
    items, cursor = pool_slice(under, waiting, 1500, 64, True, 0)
    assert (items, cursor) == ([(0, 1), (1, 1), (2, 1)], 3)
    # the tick after it (request 0's row has ended; 1 and 2 are under way): 3, passed over once, joins ahead of 1's and 2's next chunks
    items2, cursor2 = pool_slice([(1, 1, 500), (2, 1, 500)], [(1, 2, [500]), (2, 2, [500]), (3, 1, [500, 500])], 1500, 64, True, cursor)
    assert (items2, cursor2) == ([(1, 1), (2, 1), (3, 1)], 1)
    served = [{rid for rid, _ in t if (rid, _) not in seen} for t, seen in ((items, {(0, 1)}), (items2, {(1, 1), (2, 1)}))]
    assert served == [{1, 2}, {3}]


def test_empty_inputs():
    assert pool_slice([], [], 1000, 64, True, 5) == ([], 5)
    assert pool_slice([], [(1, 2, [])], None, 64, False, 5) == ([], 5)
    assert pool_slice([(1, 0, 40)], [], 1000, 64, True, 5) == ([(1, 0)], 5)
    assert pool_slice([(1, 3, 40)], [(1, 4, [])], 1000, 64, True, 5) == ([(1, 3)], 5)


def test_span_prev_gathers_rows_of_several_tensors():
    a, b = torch.arange(2 * 3 * 4, dtype=torch.float32).reshape(2, 3, 4), -torch.arange(1 * 5 * 4, dtype=torch.float32).reshape(1, 5, 4)
    assert span_prev([(None, -1), (None, -1)]) == (None, [-1, -1])
    state, rows = span_prev([(a, 1), (None, -1), (a, 0)])
    assert state is a and rows == [1, -1, 0]
    state, rows = span_prev([(a, 1), (None, -1), (b, 0)])
    assert rows == [0, -1, 1] and state.shape == (2, 5, 4)
    assert torch.equal(state[0, :3], a[1]) and (state[0, 3:] == 0).all() and torch.equal(state[1], b[0])


# ------------------------------------------------------------------------------------------------ CFM.sample_span on the host
class _Engine:
    def __init__(self):
        self.calls = []

    def sample(self, cond, cond_mask, y0, text, t_grid, cfg_strength, lens=None, want_traj=True, method="euler"):
        self.calls.append(dict(name="sample", cond=cond, cond_mask=cond_mask, y0=y0, text=text, t_grids=[t_grid] * y0.shape[0],
                               cfgs=[cfg_strength] * y0.shape[0], lens=lens, method=method))
        return torch.zeros(y0.shape), torch.zeros(len(t_grid), *y0.shape)

    def sample_items(self, cond, cond_mask, y0, text, t_grids, cfgs, lens=None, want_traj=True, method="euler"):
        self.calls.append(dict(name="sample_items", cond=cond, cond_mask=cond_mask, y0=y0, text=text, t_grids=t_grids, cfgs=cfgs, lens=lens,
                               method=method))
        return torch.zeros(y0.shape), torch.zeros(max(len(g) for g in t_grids), *y0.shape)

    def sample_span(self, cond, cond_mask, y_new, prev_state, rows, text, t_grids, cfgs, lens=None, method="euler"):
        self.calls.append(dict(name="sample_span", cond=cond, cond_mask=cond_mask, y_new=y_new, prev_state=prev_state, rows=rows, text=text,
                               t_grids=t_grids, cfgs=cfgs, lens=lens, method=method))
        state = torch.zeros(cond_mask.shape[0], cond_mask.shape[1], 100)
        return state, state


def host_model():
    m = P.CFM(transformer=P.DiT(**P.config.F5TTS_TINY, text_num_embeds=257, mel_dim=100))
    eng = _Engine()
    m.transformer.engine = lambda: eng
    m.transformer.clear_cache = lambda: None
    return m, eng


def batch():
    g = torch.Generator().manual_seed(1)
    cond = torch.randn(3, 12, 100, generator=g)
    text = torch.randint(0, 200, (3, 9), generator=g)
    return cond, text, torch.tensor([40, 21, 33]), torch.tensor([12, 7, 9])


STEPS, CFGS, SWAYS, SEEDS = [5, 2, 3], [2.0, 0.0, 0.5], [-1.0, None, -0.5], [3, None, 7]
KW = dict(steps=STEPS, cfg_strength=CFGS, sway_sampling_coef=SWAYS, seed=SEEDS)


def bits(values):
    return torch.tensor(values, dtype=torch.float32).numpy().tobytes()


def test_sub_grids_are_bitwise_slices_and_done_is_right():
    m, eng = host_model()
    cond, text, dur, lens = batch()
    full = CFM_MOD.item_time_grids(STEPS, SWAYS, True)
    res = m.sample_span(cond, text, dur, lens=lens, start=[0, 0, 0], count=2, **KW)
    assert res.done == [False, True, False] and res.state.shape == (3, 40, 100) and res.out.shape == (3, 40, 100)
    call = eng.calls[0]
    assert call["prev_state"] is None and call["rows"] == [-1, -1, -1] and call["cfgs"] == CFGS and call["lens"] == dur.tolist()
    assert [len(g) - 1 for g in call["t_grids"]] == [2, 2, 2]
    for b in range(3):
        assert bits(call["t_grids"][b]) == full[b][0:3].numpy().tobytes(), f"item {b}"
    # the second slice: item 1 has left, the batch is items 0 and 2 in the other order, N follows them
    res2 = m.sample_span(cond[[2, 0]], text[[2, 0]], dur[[2, 0]], lens=lens[[2, 0]], start=[2, 2], count=2, prev=(res.state, [2, 0]),
                         steps=[3, 5], cfg_strength=[0.5, 2.0], sway_sampling_coef=[-0.5, -1.0], seed=[7, 3])
    call = eng.calls[1]
    assert res2.done == [True, False] and call["y_new"] is None and call["prev_state"] is res.state and call["rows"] == [2, 0]
    assert bits(call["t_grids"][0]) == full[2][2:4].numpy().tobytes(), "one step is left of item 2's three"
    assert bits(call["t_grids"][1]) == full[0][2:5].numpy().tobytes()
    assert call["cond_mask"].shape == (2, 40)
    # the last step of item 0 alone: count is an upper bound
    res3 = m.sample_span(cond[:1], text[:1], dur[:1], lens=lens[:1], start=[4], count=8, prev=(res2.state, [1]), steps=5, cfg_strength=2.0,
                         sway_sampling_coef=-1.0, seed=3)
    assert res3.done == [True] and bits(eng.calls[2]["t_grids"][0]) == full[0][4:6].numpy().tobytes() and eng.calls[2]["lens"] is None


def test_a_new_rows_noise_is_item_noises_for_that_item_alone():
    m, eng = host_model()
    cond, text, dur, lens = batch()
    prev = torch.zeros(4, 40, 100)
    torch.manual_seed(123)
    m.sample_span(cond, text, dur, lens=lens, start=[0, 0, 1], count=1, prev=(prev, [-1, -1, 3]), **KW)
    y_new = eng.calls[0]["y_new"]
    torch.manual_seed(123)
    want0 = CFM_MOD.item_noise([40], [3], 100)[0]                       # seeded: its own draw
    want1 = CFM_MOD.item_noise([21], [None], 100)[0]                    # no seed: goes on from the state the item before it left
    assert y_new.shape == (3, 40, 100)
    assert torch.equal(y_new[0], want0) and torch.equal(y_new[1, :21], want1) and (y_new[1, 21:] == 0).all()
    assert (y_new[2] == 0).all(), "a continuing row draws nothing"
    # every row begins: sample_items' own noise
    m.sample_span(cond, text, dur, lens=lens, start=[0, 0, 0], count=1, **KW)
    assert torch.equal(eng.calls[1]["y_new"], CFM_MOD.item_noise(dur.tolist(), SEEDS, 100))


def test_sample_span_refusals():
    m, eng = host_model()
    cond, text, dur, lens = batch()
    prev = torch.zeros(4, 40, 100)
    ok = dict(lens=lens, start=[0, 0, 1], count=2, prev=(prev, [-1, -1, 3]), **KW)
    m.sample_span(cond, text, dur, **ok)
    for bad, match in ((dict(start=[0, 2, 1]), "item 1"),                                  # at its step count
                       (dict(start=[0, 0, 3]), "item 2"),                                  # at its step count
                       (dict(start=[0, 0, 4]), "item 2"),                                  # past it
                       (dict(start=[-1, 0, 1]), "item 0"),
                       (dict(start=[0, 1, 1]), "item 1 begins here"),                      # a -1 row starts at 0
                       (dict(prev=(torch.zeros(4, 32, 100), [-1, -1, 3])), "item 2"),      # 33 frames from a state of 32
                       (dict(prev=None, start=[0, 0, 1]), "item 2"),                       # every row -1, yet one has made steps
                       (dict(prev=(prev, [-1, -1])), "rows has 2"),
                       (dict(start=[0, 0]), "start has 2"),
                       (dict(count=0), "count"),
                       (dict(steps=[5, 2]), "steps has 2")):
        with pytest.raises(ValueError, match=match):
            m.sample_span(cond, text, dur, **{**ok, **bad})
    assert len(eng.calls) == 1, "a refused call does not reach the engine"
    with pytest.raises(TypeError):
        m.sample_span(cond, text, dur, duplicate_test=True, **ok)
    with pytest.raises(TypeError):
        m.sample_span(cond, text, dur, lens=lens, **KW)                  # start and count have no default


@pytest.mark.parametrize("no_ref_audio", [False, True])
def test_the_three_entry_points_hand_the_engine_the_same_call(no_ref_audio):
    """CFM.sample, .sample_items with scalar settings and .sample_span(start=0, count=steps) of one ragged batch: the same cond,
    cond_mask, text and lens, bitwise equal grids, equal noise."""
    m, eng = host_model()
    cond, text, dur, lens = batch()
    edit = torch.ones(3, 12, dtype=torch.bool)
    edit[0, 3:6] = edit[2, 8] = False                                   # prompt frames to re-speak: inside lens 12 and 9
    steps = 4
    kw = dict(lens=lens, steps=steps, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=5, no_ref_audio=no_ref_audio, edit_mask=edit)
    m.sample(cond, text, dur, **kw)
    m.sample_items(cond, text, dur, **kw)
    res = m.sample_span(cond, text, dur, start=[0, 0, 0], count=steps, **kw)
    assert res.done == [True] * 3
    assert [c["name"] for c in eng.calls] == ["sample", "sample_items", "sample_span"]
    want_mask = torch.zeros(3, 40, dtype=torch.bool)
    for b, n in enumerate(lens.tolist()):
        want_mask[b, :n] = edit[b, :n]
    first = eng.calls[0]
    assert first["cond_mask"].dtype == torch.bool and first["cond_mask"].shape == (3, 40) and torch.equal(first["cond_mask"], want_mask)
    assert not want_mask[0, 3:6].any() and not want_mask[2, 8] and want_mask.sum() == 12 + 7 + 9 - 4
    assert first["cond"] is None if no_ref_audio else torch.equal(first["cond"], cond)
    assert first["lens"] == [40, 21, 33] and first["cfgs"] == [2.0] * 3
    for call in eng.calls[1:]:
        assert call["cond"] is None if no_ref_audio else torch.equal(call["cond"], first["cond"]), call["name"]
        assert call["cond_mask"].dtype == torch.bool and torch.equal(call["cond_mask"], first["cond_mask"]), call["name"]
        assert call["text"].dtype == first["text"].dtype and torch.equal(call["text"], first["text"]), call["name"]
        assert call["lens"] == first["lens"] and call["cfgs"] == first["cfgs"] and call["method"] == first["method"], call["name"]
        assert [bits(g) for g in call["t_grids"]] == [bits(g) for g in first["t_grids"]], call["name"]
    assert len(first["t_grids"][0]) == steps + 1
    y_items, y_span = eng.calls[1]["y0"], eng.calls[2]["y_new"]
    assert y_items.shape == (3, 40, 100) and torch.equal(y_span, y_items) and torch.equal(first["y0"], y_items)
    assert eng.calls[2]["prev_state"] is None and eng.calls[2]["rows"] == [-1] * 3
    # B = 1: no lens for any of the three
    kw1 = dict(kw, lens=lens[:1], edit_mask=edit[:1])
    m.sample(cond[:1], text[:1], dur[:1], **kw1)
    m.sample_items(cond[:1], text[:1], dur[:1], **kw1)
    m.sample_span(cond[:1], text[:1], dur[:1], start=[0], count=steps, **kw1)
    assert [c["lens"] for c in eng.calls[3:]] == [None] * 3 and all(c["cond_mask"].shape == (1, 40) for c in eng.calls[3:])


# ------------------------------------------------------------------------------------------------ null handles
def span_call(lib, t, steps, count, cfg, rows, *, prev=None, prev_B=0, prev_N=0, y_new=None, method=0):
    B = len(steps)
    return lib.f5_sample_span(None, None, 0, None, y_new, prev, prev_B, prev_N, None if rows is None else _lib.int_array(rows), None, 1,
                              (C.c_float * len(t))(*t), _lib.int_array(steps), count, (C.c_float * len(cfg))(*cfg), None, B, 8, None, None,
                              None, method)


def test_span_refusals_are_decided_before_the_engine():
    lib = _lib.load()
    t, cfg = [0.0, 0.5, 1.0, 0.0, 1.0, 0.0], [2.0, 0.0]
    buf = (C.c_float * 4)()                                             # stands for a device address: never read, nothing is launched
    ptr = C.cast(buf, C.c_void_p)
    ok = dict(prev=ptr, prev_B=3, prev_N=8, y_new=ptr)

    def refused(rc, *words):
        msg = lib.f5_last_error()
        return rc == F5_EINVAL and all(w in msg for w in words)

    assert refused(span_call(lib, t, [2, 1], 0, cfg, [0, -1], **ok), b"count = 0")
    assert refused(span_call(lib, t, [2, 1], -3, cfg, [0, -1], **ok), b"count")
    assert refused(span_call(lib, t, [2, 0], 2, cfg, [0, -1], **ok), b"item 1")
    assert refused(span_call(lib, t, [3, 1], 2, cfg, [0, -1], **ok), b"item 0")
    assert refused(span_call(lib, t, [1, 1], 2, cfg, [0, -1], **ok), b"steps_max")
    assert refused(span_call(lib, t, [2, 1], 2, cfg, [0, 3], **ok), b"item 1", b"[-1, prev_B = 3)")
    assert refused(span_call(lib, t, [2, 1], 2, cfg, [-2, 0], **ok), b"item 0")
    assert refused(span_call(lib, t, [2, 1], 2, cfg, [2, 2], **ok), b"item 1", b"twice")
    assert refused(span_call(lib, t, [2, 1], 2, cfg, [0, -1], prev=None, prev_B=3, prev_N=8, y_new=ptr), b"item 0", b"previous state")
    assert refused(span_call(lib, t, [2, 1], 2, cfg, [0, -1], prev=ptr, prev_B=3, prev_N=8, y_new=None), b"item 1", b"y_new")
    assert refused(span_call(lib, t, [2, 1], 2, cfg, None, **ok), b"bad arguments")
    assert refused(span_call(lib, t, [2, 1], 2, cfg, [0, -1], method=7, **ok), b"unknown ODE method 7")
    # tables that pass get as far as the engine: a null handle
    assert refused(span_call(lib, t, [2, 1], 2, cfg, [0, -1], **ok), b"null engine")
    assert refused(span_call(lib, t, [2, 1], 2, cfg, [-1, -1], y_new=ptr), b"null engine")
    assert refused(span_call(lib, t, [2, 1], 2, cfg, [2, 0], prev=ptr, prev_B=3, prev_N=8), b"null engine")


def test_span_stage_refuses_null_pointers_and_bad_rows():
    lib = _lib.load()
    buf = (C.c_float * 4)()
    ptr = C.cast(buf, C.c_void_p)
    rows = _lib.int_array([1, -1])

    def stage(y=ptr, prev=ptr, prev_B=2, prev_N=5, y_new=ptr, rows_dev=ptr, rows_host=rows, B=2, N=4, mel=100):
        return lib.f5k_span_stage(y, prev, prev_B, prev_N, y_new, rows_dev, rows_host, B, N, mel, None)

    for bad in (dict(y=None), dict(rows_dev=None), dict(rows_host=None), dict(B=0), dict(N=0), dict(mel=6)):
        assert stage(**bad) == F5_EINVAL and b"f5k_span_stage" in lib.f5_last_error(), bad
    assert stage(prev=None) == F5_EINVAL and b"item 0" in lib.f5_last_error()
    assert stage(y_new=None) == F5_EINVAL and b"item 1" in lib.f5_last_error()
    assert stage(rows_host=_lib.int_array([2, -1])) == F5_EINVAL and b"item 0" in lib.f5_last_error()
    assert stage(rows_host=_lib.int_array([1, 1])) == F5_EINVAL and b"twice" in lib.f5_last_error()
    assert stage(rows_host=_lib.int_array([0, -2])) == F5_EINVAL and b"item 1" in lib.f5_last_error()


# ------------------------------------------------------------------------------------------------ the pool on the host
REF = "Some call me nature, others call me mother nature."
SENT = "The quick brown fox jumps over the lazy dog."
LONG = " ".join([SENT] * 6)


class _Bank:
    names, ref_texts, seconds, samples, frames, speeds, target_rms = ["v", "w"], [REF, REF], [3.0, 10.0], [72000, 240000], [282, 938], [None, 2.0], 0.1
    mel = torch.zeros(2, 938, 100)
    rms = torch.zeros(2)


class _Vocoder:
    def decode_ragged(self, *a, **k):
        raise AssertionError("not reached on the CPU")


class _Stop(Exception):
    pass


POOL_KW = dict(nfe_step=4, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=3)
SETTING_KEYS = ("steps", "cfg_strength", "sway_sampling_coef", "seed")


def stopping_model():
    """test_sample_items' recording model: every sampler entry point records its call and ends the tick there."""
    m = P.CFM(transformer=P.DiT(**P.config.F5TTS_TINY, text_num_embeds=257, mel_dim=100))
    calls = []

    def record(name):
        def call(*a, **kw):
            calls.append((name, kw))
            raise _Stop()
        return call

    m.sample, m.sample_items, m.sample_span = record("sample"), record("sample_items"), record("sample_span")
    return m, calls


def test_without_slice_steps_the_pool_makes_todays_calls():
    for explicit in ({}, dict(slice_steps=None)):
        m, calls = stopping_model()
        pool = I.open_pool(m, _Vocoder(), _Bank, batch_frames=20000, first_alone=False, **POOL_KW, **explicit)
        assert pool.slice_steps is None
        for voice in ("v", "w"):
            pool.connect(voice).submit(SENT)
        with pytest.raises(_Stop):
            pool._enqueue()
        (name, kw), = calls
        assert name == "sample" and set(kw) == {"cond", "text", "duration", "lens", *SETTING_KEYS}
        assert {k: kw[k] for k in SETTING_KEYS} == dict(steps=4, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=3)
        m, calls = stopping_model()
        pool = I.open_pool(m, _Vocoder(), _Bank, batch_frames=20000, first_alone=False, **POOL_KW, **explicit)
        pool.connect("v").submit(SENT)
        pool.connect("w", nfe_step=2, cfg_strength=0.5).submit(SENT)
        with pytest.raises(_Stop):
            pool._enqueue()
        (name, kw), = calls
        assert name == "sample_items" and set(kw) == {"cond", "text", "duration", "lens", *SETTING_KEYS}
        assert kw["steps"] == [4, 2] and kw["cfg_strength"] == [2.0, 0.5] and kw["seed"] == [3, 3]
        assert pool.spans == [] and len(pool.log) == 1
    for bad in (0, -2, 1.5, True, "2"):
        with pytest.raises((ValueError, TypeError)):
            I.open_pool(m, _Vocoder(), _Bank, batch_frames=20000, slice_steps=bad, **POOL_KW)


class _SlicedPool:
    """A pool with slice_steps whose model records sample_span and returns a state on the host, and whose delivery (the part of a
    tick that needs the device) records the rows it was given."""

    def __init__(self, **kw):
        self.model = P.CFM(transformer=P.DiT(**P.config.F5TTS_TINY, text_num_embeds=257, mel_dim=100))
        self.calls, self.delivered = [], []
        self.model.sample = self.model.sample_items = lambda *a, **k: pytest.fail("a sliced pool calls sample_span only")
        self.model.sample_span = self.sample_span
        self.pool = I.open_pool(self.model, _Vocoder(), _Bank, **{**POOL_KW, **kw})
        self.pool._deliver = self.deliver
        self.pool._mark = lambda: None

    def sample_span(self, **kw):
        self.calls.append(kw)
        B, N = len(kw["text"]), int(kw["duration"].max())
        state = torch.full((B, N, 100), float(len(self.calls)))
        done = [a + kw["count"] >= n for a, n in zip(kw["start"], kw["steps"])]
        return CFM_MOD.SpanResult(state + 0.5, state, done)

    def deliver(self, run, generated, rows):
        self.delivered.append(([(r.id, k) for r, k in run], generated, rows.tolist()))
        for r, k in run:
            r.pieces.append(None)
        return [], None, None

    def tick(self):
        return self.pool._enqueue_slice()


def test_a_sliced_pool_makes_the_expected_sample_span_calls():
    sp = _SlicedPool(batch_frames=20000, first_alone=False, slice_steps=2)
    pool = sp.pool
    keys = set(pool.stats())
    a, b = pool.connect("v"), pool.connect("w", nfe_step=2, cfg_strength=0.5, seed=None)
    ra, rb = a.submit(SENT), b.submit(SENT)
    assert len(ra.plan["ends"]) == 1 and len(rb.plan["ends"]) == 1 and not pool.idle()
    # tick 0: both begin; b (2 steps) ends, a (4 steps) is half way
    assert sp.tick() == ([], None, None)
    kw = sp.calls[0]
    assert set(kw) == {"cond", "text", "duration", "lens", "start", "count", "prev", *SETTING_KEYS}
    assert kw["prev"] is None and kw["start"] == [0, 0] and kw["count"] == 2
    assert kw["steps"] == [4, 2] and kw["cfg_strength"] == [2.0, 0.5] and kw["sway_sampling_coef"] == [-1.0, -1.0] and kw["seed"] == [3, None]
    assert kw["lens"].tolist() == [282, 938] and kw["cond"].shape == (2, 938, 100)
    assert pool.log == [[(ra.id, 0), (rb.id, 0)]] and pool.spans == [[(0, 2), (0, 2)]]
    (run, generated, voices), = sp.delivered
    assert run == [(rb.id, 0)] and voices == [1], "the row that ended, and only it, is delivered"
    assert generated.shape[0] == 1 and (generated == 1.5).all(), "its row of `out`"
    assert not pool.idle() and ra.under_way == 1 and rb.under_way == 0
    # a request submitted between two ticks joins the next one, behind the row under way
    rc = pool.connect("v", nfe_step=3).submit(SENT)
    sp.tick()
    kw = sp.calls[1]
    state, rows = kw["prev"]
    assert rows == [0, -1] and (state == 1.0).all() and state.shape[0] == 2, "row 0 of the first call's state; the other begins"
    assert kw["start"] == [2, 0] and kw["steps"] == [4, 3] and kw["lens"].tolist() == [282, 282] and kw["cond"].shape == (2, 282, 100)
    assert pool.log[1] == [(ra.id, 0), (rc.id, 0)] and pool.spans[1] == [(2, 2), (0, 2)]
    assert sp.delivered[1][0] == [(ra.id, 0)]
    # the last step of the late request, alone
    sp.tick()
    kw = sp.calls[2]
    assert kw["prev"][1] == [1] and (kw["prev"][0] == 2.0).all() and kw["start"] == [2] and kw["steps"] == [3]
    assert pool.log[2] == [(rc.id, 0)] and pool.spans[2] == [(2, 1)] and sp.delivered[2][0] == [(rc.id, 0)]
    assert len(sp.delivered[2][1]) == 1
    assert sp.tick() is None and pool.idle()
    # rows / start are consistent with the log and the spans, tick by tick
    place, made = {}, {}
    for kw, items, spans in zip(sp.calls, pool.log, pool.spans):
        rows = [-1] * len(items) if kw["prev"] is None else kw["prev"][1]
        for b, (item, (start, run)) in enumerate(zip(items, spans)):
            assert rows[b] == place.get(item, -1) and kw["start"][b] == start == made.get(item, 0), (item, b)
            made[item] = start + run
        place = {item: b for b, item in enumerate(items)}
    assert made == {(ra.id, 0): 4, (rb.id, 0): 2, (rc.id, 0): 3}
    stats = pool.stats()
    assert set(stats) == keys == {"ticks", "sample_calls", "decode_calls", "emit_launches", "copies", "packets", "prompt_passes"}
    assert stats["ticks"] == stats["sample_calls"] == 3


def test_a_tick_that_ends_no_row_delivers_nothing():
    sp = _SlicedPool(batch_frames=20000, first_alone=False, slice_steps=1)
    r = sp.pool.connect("v").submit(SENT)
    for n in range(3):
        assert sp.tick() == ([], None, None) and sp.delivered == [] and not sp.pool.idle() and r.under_way == 1, n
    sp.tick()
    assert [d[0] for d in sp.delivered] == [[(r.id, 0)]] and sp.pool.idle() and r.under_way == 0
    assert sp.pool.spans == [[(0, 1)], [(1, 1)], [(2, 1)], [(3, 1)]] and sp.pool.stats()["ticks"] == 4


def test_a_first_chunk_parks_the_long_rows_in_the_pool():
    sp = _SlicedPool(batch_frames=20000, first_alone=True, slice_steps=1, nfe_step=3)
    pool = sp.pool
    a = pool.connect("v")
    ra = a.submit(LONG)
    assert len(ra.plan["ends"]) >= 3
    sp.tick()                                                            # a's first chunk, alone
    sp.tick()
    sp.tick()
    assert pool.log == [[(ra.id, 0)]] * 3 and sp.delivered[0][0] == [(ra.id, 0)]
    sp.tick()                                                            # its later chunks begin
    later = [(ra.id, k) for k in range(1, len(ra.plan["ends"]))]
    assert pool.log[3] == later
    rb = pool.connect("w").submit(SENT)                                  # a first chunk arrives while they are under way
    for n in range(3):
        sp.tick()
        assert pool.log[-1] == [(rb.id, 0)], "the long rows are parked"
        assert sp.calls[-1]["start"] == [n] and (sp.calls[-1]["prev"] is None) == (n == 0)
    assert sp.delivered[-1][0] == [(rb.id, 0)] and ra.under_way == len(later)
    sp.tick()                                                            # they resume where they were, from the state they left
    kw = sp.calls[-1]
    assert pool.log[-1][:len(later)] == later and kw["start"][:len(later)] == [1] * len(later)
    state, rows = kw["prev"]
    assert rows[:len(later)] == list(range(len(later))) and (state == 4.0).all(), "the state of the tick they last ran in"
    assert pool.spans[-1][:len(later)] == [(1, 1)] * len(later)
