"""CPU: isolated rows as far as they go without a device -- the numpy restatement of the packed per-item updates against a literal
per-element loop, the packed budget of pool_tick / pool_slice against hand-computed ticks and as properties over the seeded queues
of test_stream_pool.py, the default budget unchanged, the new symbols in the header and the library, and the refusal of a backbone
without packed rows."""
import copy
import os
import random
import re

import numpy as np
import pytest

import isolate_oracle as ISO
from conftest import ROOT
from test_stream_pool import _Bank, _Vocoder, model, random_queue

import f5_tts_amd as P
from f5_tts_amd import _lib
from f5_tts_amd import infer as I
from f5_tts_amd import stream as S

F32 = np.float32


# ------------------------------------------------------------------------------------------------ the oracle
def literal_update(y, pred, rs, lens, t, cfg, steps, step, use_cfg, half):
    B, N, mel = y.shape
    out = y.copy()
    for b in range(B):
        for n in range(N):
            for c in range(mel):
                if not (step < steps[b] and n < lens[b]):
                    continue
                dt = F32(F32(t[b][step + 1]) - F32(t[b][step]))
                p = F32(pred[rs[b] + n, c])
                v = p
                if use_cfg and not F32(cfg[b]) < F32(1e-5):
                    u = F32(pred[rs[B + b] + n, c])
                    v = F32(p + F32(F32(p - u) * F32(cfg[b])))
                if half:
                    out[b, n, c] = F32(y[b, n, c] + F32(v * F32(F32(0.5) * dt)))
                else:
                    out[b, n, c] = F32(y[b, n, c] + F32(dt * v))
    return out


@pytest.mark.parametrize("use_cfg", [1, 0])
def test_the_oracle_against_a_literal_loop(use_cfg):
    rng = np.random.default_rng(11)
    lens, steps, cfg = [7, 2, 1], [2, 1, 2], [1.5, 0.0, 0.3]
    rs = ISO.row_start(lens, 2 if use_cfg else 1)
    assert rs.tolist() == ([0, 8, 12, 16, 24, 28, 32] if use_cfg else [0, 8, 12, 16])
    y = rng.standard_normal((3, 7, 8)).astype(F32)
    pred = rng.standard_normal((int(rs[-1]), 8)).astype(F32)
    t = np.sort(rng.random((3, 3)).astype(F32), axis=1)
    for step in (0, 1):
        for half, fn in ((False, ISO.euler_items_packed), (True, ISO.midpoint_half_items_packed)):
            got = fn(y, pred, rs, lens, t, cfg, steps, step, use_cfg)
            assert got.dtype == F32 and got.tobytes() == literal_update(y, pred, rs, lens, t, cfg, steps, step, use_cfg, half).tobytes()
            assert np.array_equal(got[1, 2:], y[1, 2:]) and np.array_equal(got[2, 1:], y[2, 1:]), "frames past an item's length"
            assert not np.array_equal(got[0], y[0])
            if step == 1:
                assert np.array_equal(got[1], y[1]), "a finished item"


def test_the_staging_oracle():
    rng = np.random.default_rng(3)
    prev, y_new = rng.standard_normal((2, 3, 4)).astype(F32), rng.standard_normal((2, 5, 4)).astype(F32)
    y = np.full((2, 8, 4), 9.0, F32)
    got = ISO.span_stage_pitched(y, prev, y_new, [1, -1], 5)
    assert np.array_equal(got[0, :3], prev[1]) and (got[0, 3:5] == 0).all() and np.array_equal(got[1, :5], y_new[1]) and (got[:, 5:] == 9.0).all()


# ------------------------------------------------------------------------------------------------ the packed budget
def test_packed_ticks_hand_computed():
    assert S.tick_cost([300] + [1000] * 15, True) == 15300 and S.tick_cost([300] + [1000] * 15, False) == 16000
    assert S.tick_cost([41, 3], True) == 48 and S.tick_cost([], True) == 0
    # rows x longest row keeps 150 out of a budget of 299; the sum of the rows (100 + 152) takes it at 252 and not at 251
    q = [(0, 1, [100]), (1, 1, [150])]
    assert S.pool_tick(q, 299, 64, True, 0) == ([(0, 1)], 1)
    assert S.pool_tick(q, 252, 64, True, 0, packed=True) == ([(0, 1), (1, 1)], 0)
    assert S.pool_tick(q, 251, 64, True, 0, packed=True) == ([(0, 1)], 1)
    # a short first chunk beside long rows: the rectangle charges it 1,000 frames, the packed tick 300
    q = [(0, 1, [300]), (1, 1, [1000]), (2, 1, [1000])]
    assert S.pool_tick(q, 2300, 64, True, 0) == ([(0, 1), (1, 1)], 2)
    assert S.pool_tick(q, 2300, 64, True, 0, packed=True) == ([(0, 1), (1, 1), (2, 1)], 0)
    # an item over the budget runs alone, nothing overtakes the item that did not fit, max_items still holds, first chunks first
    assert S.pool_tick([(0, 1, [900, 10]), (1, 1, [10])], 400, 64, True, 0, packed=True) == ([(0, 1)], 1)
    assert S.pool_tick([(0, 1, [100]), (1, 1, [900]), (2, 1, [100])], 400, 64, True, 0, packed=True) == ([(0, 1)], 1)
    assert S.pool_tick(q, None, 2, True, 0, packed=True) == ([(0, 1), (1, 1)], 2)
    waiting = [(3, 1, [100, 100]), (5, 0, [50, 100]), (9, 0, [60])]
    assert S.pool_tick(waiting, 400, 64, True, 3, packed=True) == ([(5, 0), (9, 0)], 3)
    assert S.pool_tick(waiting, 111, 64, True, 3, packed=True) == ([(5, 0)], 3)           # 52 + 60 = 112
    assert S.pool_tick(waiting, 112, 64, True, 3, packed=True) == ([(5, 0), (9, 0)], 3)
    # pool_slice: rows under way first, then the waiting chunks, under the same sum
    under = [(1, 1, 1000), (2, 1, 1000)]
    assert S.pool_slice(under, [(4, 1, [300])], 2300, 64, True, 0) == ([(1, 1), (2, 1)], 4)
    assert S.pool_slice(under, [(4, 1, [300])], 2300, 64, True, 0, packed=True) == ([(1, 1), (2, 1), (4, 1)], 0)
    assert S.pool_slice(under, [(4, 1, [300])], 1999, 64, True, 0, packed=True) == ([(1, 1)], 0)   # a row under way that does not fit
    assert S.pool_slice([(1, 0, 100), (2, 1, 50)], [(4, 0, [41])], 143, 64, True, 0, packed=True) == ([(1, 0)], 0)   # 100 + 44
    assert S.pool_slice([(1, 0, 100), (2, 1, 50)], [(4, 0, [41])], 144, 64, True, 0, packed=True) == ([(1, 0), (4, 0)], 0)


@pytest.mark.parametrize("seed", range(40))
def test_packed_tick_properties_over_random_queues(seed):
    """test_stream_pool.py's queues and its properties -- progress, order inside a request, first chunks first, the fairness bound --
    under the packed budget."""
    rng = random.Random(seed)
    queue = random_queue(rng)
    batch_frames, max_items = rng.choice([None, 100, 300, 600, 2000]), rng.choice([1, 2, 3, 8, 64])
    first_alone, cursor = rng.random() < 0.7, rng.randint(0, 12)
    previous, ticks, left = None, 0, sum(len(w[2]) for w in queue)
    while queue:
        before = copy.deepcopy(queue)
        items, new_cursor = S.pool_tick(queue, batch_frames, max_items, first_alone, cursor, packed=True)
        assert queue == before, "pool_tick changed its input"
        # the same queue as rows under way: pool_slice takes them in their order under the same budget
        frames_of = {(rid, k + j): f for rid, k, fr in queue for j, f in enumerate(fr)}
        assert items and len(set(items)) == len(items) and all(it in frames_of for it in items), "no progress, or an item that does not wait"
        rows = len(items)
        assert rows <= max_items
        assert rows == 1 or batch_frames is None or S.tick_cost([frames_of[it] for it in items], True) <= batch_frames, (items, batch_frames)
        assert S.pool_slice([], queue, batch_frames, max_items, first_alone, cursor, packed=True) == (items, new_cursor), "no row under way: pool_tick"
        for rid, k, _ in queue:
            own = [c for r, c in items if r == rid]
            assert own == list(range(k, k + len(own))), (rid, k, own)
        firsts = [rid for rid, k, _ in queue if k == 0]
        round_robin = not (first_alone and firsts)
        if not round_robin:
            assert all(k == 0 for _, k in items) and [r for r, _ in items] == firsts[:rows] and new_cursor == cursor
        served, waited = {r for r, _ in items}, {rid for rid, _, _ in queue}
        if round_robin and previous is not None:
            for x in (previous["waited"] & waited) - previous["served"] - served:
                assert not (previous["served"] & served), f"request {x} was passed over twice in a row for {previous['served'] & served}"
        previous = dict(served=served, waited=waited) if round_robin else None
        queue = [(rid, k + sum(1 for r, _ in items if r == rid), fr[sum(1 for r, _ in items if r == rid):]) for rid, k, fr in queue]
        queue = [w for w in queue if w[2]]
        cursor, ticks, left = new_cursor, ticks + 1, left - rows
        if rng.random() < 0.25 and ticks < 30:
            more = random_queue(rng, first_id=max([w[0] for w in queue], default=cursor) + 1)[:2]
            queue, left = queue + more, left + sum(len(w[2]) for w in more)
    assert left == 0


@pytest.mark.parametrize("seed", range(10))
def test_the_default_ticks_are_unchanged(seed):
    """packed=False is the default, and is the rows x longest row rule: against a restatement of that rule's budget."""
    rng = random.Random(100 + seed)
    for _ in range(20):
        queue = random_queue(rng)
        batch_frames, max_items = rng.choice([None, 100, 300, 600, 2000]), rng.choice([1, 2, 3, 8, 64])
        first_alone, cursor = rng.random() < 0.7, rng.randint(0, 12)
        got = S.pool_tick(queue, batch_frames, max_items, first_alone, cursor)
        assert got == S.pool_tick(queue, batch_frames, max_items, first_alone, cursor, packed=False)
        assert got == S.pool_slice([], queue, batch_frames, max_items, first_alone, cursor)
        frames_of = {(rid, k + j): f for rid, k, fr in queue for j, f in enumerate(fr)}
        taken = [frames_of[it] for it in got[0]]
        assert len(taken) == 1 or batch_frames is None or len(taken) * max(taken) <= batch_frames
        under = [(rid, k, fr[0]) for rid, k, fr in queue]
        assert S.pool_slice(under, [], batch_frames, max_items, first_alone, cursor) == \
            S.pool_slice(under, [], batch_frames, max_items, first_alone, cursor, packed=False)
    waiting = [(3, 1, [100, 100]), (5, 2, [100]), (9, 1, [100, 100, 100])]
    assert S.pool_tick(waiting, 400, 64, True, 0) == ([(3, 1), (5, 2), (9, 1), (3, 2)], 9)


# ------------------------------------------------------------------------------------------------ the ABI and the Python surface
NEW = ["f5_set_isolated_rows", "f5_set_graph_capacity", "f5k_euler_cfg_items_packed", "f5k_midpoint_half_cfg_items_packed",
       "f5k_span_stage_pitched"]


def test_the_new_symbols_are_declared_exported_and_refuse_null_handles():
    src = open(os.path.join(ROOT, "include", "f5_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _lib.load()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), f"{name} is not declared in include/f5_hip.h"
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert lib.f5_set_isolated_rows(None, 1) == -1 and b"f5_set_isolated_rows" in lib.f5_last_error()
    assert lib.f5_set_graph_capacity(None, 32) == -1 and b"f5_set_graph_capacity" in lib.f5_last_error()
    # the existing signature of the staging entry point is as it was
    assert re.search(r"int f5k_span_stage\(float\* y, const float\* prev_state, int32_t prev_B, int32_t prev_N, const float\* y_new, "
                     r"const int32_t\* rows,\s+const int32_t\* rows_host, int32_t B, int32_t N, int32_t mel, f5_stream stream\);", src)


def test_the_engine_switches_without_a_device():
    import ctypes as C
    lib = _lib.load()
    cfg = _lib.f5_config()
    cfg.dim, cfg.depth, cfg.heads, cfg.dim_head, cfg.ff_dim, cfg.text_dim, cfg.mel_dim = 256, 2, 4, 64, 512, 64, 100
    cfg.text_num_embeds, cfg.max_pos = 40, 512
    h = C.c_void_p()
    assert lib.f5_create(C.byref(cfg), C.byref(h)) == 0, lib.f5_last_error()
    try:
        assert lib.f5_set_isolated_rows(h, 1) == 0 and lib.f5_set_isolated_rows(h, 0) == 0
        for n in (16, 40, 64):
            assert lib.f5_set_graph_capacity(h, n) == 0
        for n in (0, 15, 65, -1):
            assert lib.f5_set_graph_capacity(h, n) == -1 and str(n).encode() in lib.f5_last_error()
    finally:
        lib.f5_destroy(h)


def test_the_model_switch_and_the_pool_without_a_device():
    m = model()
    tr = m.transformer
    assert tr.isolated_rows is False and tr.graph_capacity == 0
    tr.set_isolated_rows(True)
    assert tr.isolated_rows is True
    tr.set_isolated_rows(False)
    for bad in (15, 65):
        with pytest.raises(ValueError, match="graph capacity"):
            tr.set_graph_capacity(bad)
    plain = I.open_pool(m, _Vocoder(), _Bank, batch_frames=1000, nfe_step=2)
    assert plain.isolate is False and "isolated" not in plain.stats() and tr.isolated_rows is False and tr.graph_capacity == 0
    pool = I.open_pool(m, _Vocoder(), _Bank, batch_frames=1000, nfe_step=2, isolate=True)
    assert pool.isolate is True and pool.stats()["isolated"] is True and tr.isolated_rows is True and tr.graph_capacity == 64
    assert pool.step() == [] and pool.stats()["ticks"] == 0
    loaded = I.load_model(P.DiT, dict(P.config.F5TTS_TINY), None, device="cpu", isolated_rows=True)
    assert loaded.transformer.isolated_rows is True
    assert I.load_model(P.DiT, dict(P.config.F5TTS_TINY), None, device="cpu").transformer.isolated_rows is False


def test_open_pool_isolate_on_a_unett_model_raises():
    e2 = dict(dim=256, depth=4, heads=4, dim_head=64, ff_mult=2, text_mask_padding=False, pe_attn_head=1)
    m = P.CFM(transformer=P.UNetT(**e2, text_num_embeds=257, mel_dim=100))
    with pytest.raises(NotImplementedError, match="isolated rows"):
        I.open_pool(m, _Vocoder(), _Bank, batch_frames=1000, nfe_step=2, isolate=True)
    with pytest.raises(NotImplementedError, match="isolated rows"):
        m.transformer.set_isolated_rows(True)
    assert m.transformer.isolated_rows is False
    I.open_pool(m, _Vocoder(), _Bank, batch_frames=1000, nfe_step=2)     # without isolate it opens as before
