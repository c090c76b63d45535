"""GPU: sliced ODE solves (f5_sample_span; CFM.sample_span; a pool with slice_steps).

The yardsticks: a chain of slices at fixed composition is the unsliced f5_sample_items solve bit for bit; a slice over a re-formed
batch (rows left, rows joined, another N, another row order) is, bit for bit, the engine's own sample_items on the same sub-grids
from a start state that torch builds out of the previous state; on an attn_mask_enabled engine, whose items do not depend on
their batch, every item is the float64 oracle's solve of that item alone.  Tiny architectures of the committed fixtures."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import items_oracle as IO  # noqa: E402
from conftest import load_golden, synthetic_weights  # noqa: E402
from gpu_util import DEV, Guarded, _a, _p, _s, k_gemm_plan  # noqa: E402
from oracle import f5_oracle as O  # noqa: E402
from test_sample_items_gpu import TOL, build, cached, columns, dev, inputs  # noqa: E402

import f5_tts_amd as P  # noqa: E402
from f5_tts_amd import _lib  # noqa: E402
from f5_tts_amd import cfm as CFM_MOD  # noqa: E402
from f5_tts_amd import infer as I  # noqa: E402
from f5_tts_amd.stream import span_prev  # noqa: E402
from f5_tts_amd.utils import lens_to_mask  # noqa: E402

NAN = float("nan")


def sub_grids(settings, start, count):
    """The slices CFM.sample_span takes of the items' grids, as lists, and the steps each item makes."""
    full = CFM_MOD.item_time_grids([s[0] for s in settings], [s[2] for s in settings])
    run = [min(count, s[0] - a) for s, a in zip(settings, start)]
    return [t[a:a + r + 1].tolist() for t, a, r in zip(full, start, run)], run


def time_rows(settings, start, count, method):
    grids, run = sub_grids(settings, start, count)
    return len(IO.item_time_rows(grids, run, method)[0])


def time_path_plans_alike(fixture, row_counts):
    meta, _ = load_golden(fixture)
    D = meta["arch"]["dim"]
    shapes = [(D, 256), (D, D)] + ([((6 * meta["arch"]["depth"] + 2) * D, D)] if meta.get("backbone", "DiT") == "DiT" else [])
    for n, k in shapes:     # the GEMMs of the time path, f32
        tiles = {m: [(fam, tile) for fam, tile, _, _ in k_gemm_plan(4, m, n, k)] for m in sorted(set(row_counts))}
        assert len({str(t) for t in tiles.values()}) == 1, f"the time path's [{n} x {k}] GEMM plans its row counts differently: {tiles}"


# ------------------------------------------------------------------------------------------------ 1. a chain is the unsliced solve
CH_DURS, CH_REFS, CH_NTS = [129, 17, 66, 40], [30, 6, 20, 12], [12, 5, 9, 7]     # 129 crosses a 128-row tile and a 64-key tile
CH_SET = [(4, 2.0, -1.0, 3), (4, 0.0, -0.5, 5), (4, 0.5, -1.0, 3), (4, 2.0, -0.5, 9)]
CHAINS = ([3, 1], [1, 1, 1, 1])


def chain_case(fixture, prec, method):
    """sample_items against every chain of CHAINS, at fixed composition and row order."""
    counts = {time_rows(CH_SET, [0] * 4, 4, method)}
    for chain in CHAINS:
        at = 0
        for count in chain:
            counts.add(time_rows(CH_SET, [at] * 4, count, method))
            at += count
    assert len(counts) > 2, "the slices have other row counts than the whole solve: the check below is not empty"
    time_path_plans_alike(fixture, counts)
    cond, text, dur, lens = inputs(CH_DURS, CH_REFS, CH_NTS)
    model = build(fixture, prec, method)
    want_out, want_traj = model.sample_items(cond, text, dur, lens=lens, **columns(CH_SET))
    for chain in CHAINS:
        prev, at = None, 0
        for count in chain:
            res = model.sample_span(cond, text, dur, lens=lens, start=[at] * 4, count=count, prev=prev, **columns(CH_SET))
            at += count
            assert res.done == [at == 4] * 4
            assert torch.equal(res.state, want_traj[at]), f"{prec} {method} chain {chain}: the state behind step {at}"
            prev = (res.state, [0, 1, 2, 3])
        assert torch.equal(res.out, want_out), f"{prec} {method} chain {chain}: out"


@pytest.mark.parametrize("prec", ["f32", "f16p"])
@pytest.mark.parametrize("method", ["euler", "midpoint"])
def test_a_chain_at_fixed_composition_is_the_unsliced_solve_bit_for_bit(method, prec):
    chain_case("sample_b1_nfe16", prec, method)


# ------------------------------------------------------------------------------------------------ 7. UNetT
def test_unett_chain_is_the_unsliced_solve_bit_for_bit():
    chain_case("sample_unett_b2", "f16x3", "euler")


# ------------------------------------------------------------------------------------------------ 2 - 3. the batch is re-formed
RF_DURS, RF_REFS, RF_NTS = [66, 129, 17, 40], [20, 30, 6, 12], [9, 12, 5, 7]
# (steps, cfg, sway, seed)
RF_SET = [(4, 2.0, -1.0, 3), (2, 0.0, None, 5), (4, 0.5, -1.0, 3), (3, 2.0, -0.5, 9)]


def engine_inputs(cond, text, dur, lens, keep):
    """What CFM hands the engine for the items `keep` of a batch: cond, cond_mask [B, N], text, durations, N."""
    durs = [int(dur[i]) for i in keep]
    N = max(durs)
    mask = torch.nn.functional.pad(lens_to_mask(lens[keep]), (0, N - int(lens[keep].max())), value=False)
    return cond[keep], mask, text[keep], durs, N


@pytest.mark.parametrize("prec", ["f32", "f16p"])
@pytest.mark.parametrize("method", ["euler", "midpoint"])
def test_rows_leave_and_n_shrinks(method, prec):
    """count = 2: the 129-frame item ends in the first call; the second runs the other three at N = 66.  The yardstick is the
    engine's own sample_items on the same sub-grids, its y0 built by torch from the previous state."""
    cond, text, dur, lens = inputs(RF_DURS, RF_REFS, RF_NTS)
    eng = build("sample_b1_nfe16", prec, method).transformer.engine()
    cfgs = [s[1] for s in RF_SET]
    y0 = CFM_MOD.item_noise(RF_DURS, [s[3] for s in RF_SET], 100)
    # ---- first call: every row begins
    c, mask, tx, durs, N = engine_inputs(cond, text, dur, lens, [0, 1, 2, 3])
    grids, run = sub_grids(RF_SET, [0] * 4, 2)
    assert N == 129 and run == [2, 2, 2, 2]
    want_out, want_traj = eng.sample_items(c, mask, y0, tx, grids, cfgs, lens=durs, method=method)
    out, state = eng.sample_span(c, mask, y0, None, [-1] * 4, tx, grids, cfgs, lens=durs, method=method)
    assert torch.equal(state, want_traj[-1]) and torch.equal(out, want_out), "first slice"
    # ---- second call: items 0, 2, 3 at N = 66
    keep = [0, 2, 3]
    c, mask, tx, durs, N = engine_inputs(cond, text, dur, lens, keep)
    grids, run = sub_grids([RF_SET[i] for i in keep], [2, 2, 2], 2)
    assert N == 66 and run == [2, 2, 1]
    y_start = state.index_select(0, torch.tensor(keep, device=DEV))[:, :N].contiguous()
    want_out, want_traj = eng.sample_items(c, mask, y_start, tx, grids, [cfgs[i] for i in keep], lens=durs, method=method)
    prev = state.clone()
    prev[1] = NAN                                                       # the row that left
    prev[:, N:] = NAN                                                   # the frames the smaller batch drops
    out2, state2 = eng.sample_span(c, mask, None, prev, keep, tx, grids, [cfgs[i] for i in keep], lens=durs, method=method)
    assert state2.shape == (3, 66, 100) and torch.isfinite(state2).all()
    assert torch.equal(state2, want_traj[-1]) and torch.equal(out2, want_out), "second slice"
    assert not torch.equal(state2[0], y_start[0]), "the steps do move the state"


@pytest.mark.parametrize("prec", ["f32", "f16p"])
@pytest.mark.parametrize("method", ["euler", "midpoint"])
def test_a_row_joins_and_n_grows(method, prec):
    """The 17- and 40-frame items run two steps at N = 40; then the 129-frame item joins between them, in another row order."""
    cond, text, dur, lens = inputs(RF_DURS, RF_REFS, RF_NTS)
    eng = build("sample_b1_nfe16", prec, method).transformer.engine()
    first = [2, 3]
    c, mask, tx, durs, N = engine_inputs(cond, text, dur, lens, first)
    grids, run = sub_grids([RF_SET[i] for i in first], [0, 0], 2)
    y0 = CFM_MOD.item_noise(durs, [RF_SET[i][3] for i in first], 100)
    _, state = eng.sample_span(c, mask, y0, None, [-1, -1], tx, grids, [RF_SET[i][1] for i in first], lens=durs, method=method)
    assert state.shape == (2, 40, 100)
    order = [3, 1, 2]                                                   # rows of the new batch: item 3 (row 1 before), the joiner, item 2 (row 0)
    c, mask, tx, durs, N = engine_inputs(cond, text, dur, lens, order)
    grids, run = sub_grids([RF_SET[i] for i in order], [2, 0, 2], 2)
    assert N == 129 and run == [1, 2, 2]
    cfgs = [RF_SET[i][1] for i in order]
    noise = CFM_MOD.item_noise([129], [RF_SET[1][3]], 100).to(DEV)
    y_start = torch.zeros(3, N, 100, device=DEV)
    y_start[0, :40], y_start[1], y_start[2, :40] = state[1], noise[0], state[0]      # frames 40 .. 128 of the two begin as zero
    want_out, want_traj = eng.sample_items(c, mask, y_start, tx, grids, cfgs, lens=durs, method=method)
    y_new = torch.full((3, N, 100), NAN, device=DEV)                    # the rows of continuing items are not read
    y_new[1] = noise[0]
    out, new_state = eng.sample_span(c, mask, y_new, state, [1, -1, 0], tx, grids, cfgs, lens=durs, method=method)
    assert torch.isfinite(new_state).all()
    assert torch.equal(new_state, want_traj[-1]) and torch.equal(out, want_out)


# ------------------------------------------------------------------------------------------------ 4. against the float64 oracle
MASKED = "sample_b3_attnmask"


def oracle_items():
    """The oracle's solve of every item of RF_SET alone (B = 1, its own prompt, text, noise and settings): (out, final state)."""
    def make():
        meta, _ = load_golden(MASKED)
        assert meta["arch"]["attn_mask_enabled"]
        sd = cached(("sd", MASKED), lambda: synthetic_weights(meta))
        cond, text, dur, lens = inputs(RF_DURS, RF_REFS, RF_NTS)
        want = []
        for i, (steps, cfg, sway, seed) in enumerate(RF_SET):
            y0 = CFM_MOD.item_noise([RF_DURS[i]], [seed], 100)
            out, traj = O.sample(sd, meta["arch"], cond[i:i + 1, :RF_REFS[i]], text[i:i + 1, :RF_NTS[i]], RF_DURS[i], steps=steps,
                                 cfg_strength=cfg, sway_sampling_coef=sway, y0=y0)
            want.append((out[0], traj[-1, 0]))
        return want
    return cached("span oracle items", make)


@pytest.mark.parametrize("prec", ["f32", "f16p", "f16", "bf16"])
def test_a_re_formed_batch_against_the_oracle_item_by_item(prec):
    """test_rows_leave_and_n_shrinks' scenario through CFM.sample_span on an attn_mask_enabled engine: an item does not see its
    batch there, so each is the oracle's solve of that item alone, inside its own frames."""
    cond, text, dur, lens = inputs(RF_DURS, RF_REFS, RF_NTS)
    model = build(MASKED, prec)
    first = model.sample_span(cond, text, dur, lens=lens, start=[0] * 4, count=2, **columns(RF_SET))
    assert first.done == [False, True, False, False] and first.state.shape == (4, 129, 100)
    keep = [0, 2, 3]
    second = model.sample_span(cond[keep], text[keep], dur[keep], lens=lens[keep], start=[2] * 3, count=2, prev=(first.state, keep),
                               **columns([RF_SET[i] for i in keep]))
    assert second.done == [True] * 3 and second.state.shape == (3, 66, 100)
    got = {1: (first.out[1], first.state[1]), 0: (second.out[0], second.state[0]), 2: (second.out[1], second.state[1]),
           3: (second.out[2], second.state[2])}
    for i, (want_out, want_state) in enumerate(oracle_items()):
        n = RF_DURS[i]
        e_out = (got[i][0][:n].cpu() - want_out).abs().max().item()
        e_state = (got[i][1][:n].cpu() - want_state).abs().max().item()
        print(f"[span {prec}] item {i} {RF_SET[i]}: state Linf {e_state:.3e} out Linf {e_out:.3e}")
        assert e_out < TOL[prec] and e_state < TOL[prec], f"item {i}"


# ------------------------------------------------------------------------------------------------ 5. the staging kernel
def stage_want(prev, y_new, rows, N):
    B, mel = len(rows), prev.shape[2]
    want = np.zeros((B, N, mel), np.float32)
    for b, r in enumerate(rows):
        if r < 0:
            want[b] = y_new[b]
        else:
            n = min(N, prev.shape[1])
            want[b, :n] = prev[r, :n]
    return want


@pytest.mark.parametrize("N,prev_N,rows", [(5, 7, [3, -1, 0, 2]),          # N < prev_N: the tail is dropped
                                           (7, 5, [2, 0, -1, 3, 1]),       # N > prev_N: new frames are +0.0; 875 float4, four blocks
                                           (5, 5, [1, 0]),                 # one block, not full
                                           (3, 4, [-1, -1, -1]),           # no row continues
                                           (11, 11, [0, 1, 2, 3])])        # the identity
def test_span_stage_is_bit_exact(N, prev_N, rows):
    lib = _lib.load()
    B, prev_B, mel = len(rows), 4, 100
    assert (B * N * mel // 4) % 256 != 0, "not a multiple of the block"
    rng = np.random.default_rng(N * 100 + prev_N)
    prev = rng.standard_normal((prev_B, prev_N, mel)).astype(np.float32)
    y_new = rng.standard_normal((B, N, mel)).astype(np.float32)
    for b, r in enumerate(rows):
        if r >= 0:
            y_new[b] = np.nan                                           # never read
    for r in set(range(prev_B)) - set(rows):
        prev[r] = np.nan                                                # never read
    y, prev_dev, new_dev, rows_dev = Guarded((B, N, mel), torch.float32), dev(prev), dev(y_new), dev(rows, torch.int32)
    _lib.check(lib.f5k_span_stage(_a(y), _p(prev_dev), prev_B, prev_N, _p(new_dev), _p(rows_dev), _lib.int_array(rows), B, N, mel, _s()),
               "f5k_span_stage")
    want = stage_want(prev, y_new, rows, N)
    assert not np.isnan(want).any()
    assert y.guards_intact() and y.value.cpu().numpy().tobytes() == want.tobytes()
    # a null y_new where nothing begins, a null prev_state where nothing continues
    if all(r >= 0 for r in rows) or all(r < 0 for r in rows):
        y = Guarded((B, N, mel), torch.float32)
        none_new = all(r >= 0 for r in rows)
        _lib.check(lib.f5k_span_stage(_a(y), None if not none_new else _p(prev_dev), prev_B if none_new else 0, prev_N if none_new else 0,
                                      None if none_new else _p(new_dev), _p(rows_dev), _lib.int_array(rows), B, N, mel, _s()), "f5k_span_stage")
        assert y.guards_intact() and y.value.cpu().numpy().tobytes() == want.tobytes()


def test_span_stage_refusals_launch_nothing():
    lib = _lib.load()
    y, prev, new, rows_dev = Guarded((2, 4, 100), torch.float32), torch.zeros(2, 5, 100, device=DEV), torch.zeros(2, 4, 100, device=DEV), dev([1, -1], torch.int32)

    def stage(rows_host, prev_t=prev, new_t=new, mel=100):
        return lib.f5k_span_stage(_a(y), _p(prev_t), 2, 5, _p(new_t), _p(rows_dev), _lib.int_array(rows_host), 2, 4, mel, _s())

    for rows_host, kw, word in (([2, -1], {}, b"item 0"), ([0, -2], {}, b"item 1"), ([1, 1], {}, b"twice"), ([1, -1], dict(prev_t=None), b"item 0"),
                                ([1, -1], dict(new_t=None), b"item 1"), ([1, -1], dict(mel=6), b"mel")):
        assert stage(rows_host, **kw) == -1 and word in lib.f5_last_error(), word
    torch.cuda.synchronize()
    assert torch.isnan(y.value).all() and y.guards_intact(), "a refused call writes nothing"
    assert stage([1, -1]) == 0


def test_engine_refusals_stage_nothing():
    model = build("sample_b1_nfe16", "f32")
    eng = model.transformer.engine()
    cond, text, dur, lens = inputs([20, 12], [6, 4], [5, 3])
    mask, y_new, prev = torch.zeros(2, 20, dtype=torch.bool), torch.zeros(2, 20, 100), torch.zeros(3, 20, 100)
    grids = [[0.0, 0.5, 1.0], [0.0, 1.0]]
    ok = dict(lens=[20, 12])
    for rows, kw, match in (([0, 3], {}, r"item 1: rows = 3 outside \[-1, prev_B = 3\)"), ([2, 2], {}, "twice"), ([0, -1], dict(prev=None), "item 0"),
                            ([0, -1], dict(y_new=None), "item 1"), ([0, -1], dict(lens=None), "lens required"),
                            ([0, -1], dict(lens=[20, 21]), r"lens\[1\]=21"), ([0, -1], dict(cfgs=[2.0, NAN]), "item 1")):
        a = dict(prev=prev, y_new=y_new, cfgs=[2.0, 2.0], **ok)
        a.update(kw)
        with pytest.raises(_lib.F5Error, match=match):
            eng.sample_span(cond, mask, a["y_new"], a["prev"], rows, text, grids, a["cfgs"], lens=a["lens"])
    with pytest.raises(ValueError):
        eng.sample_span(cond, mask, y_new, prev, [0], text, grids, [2.0, 2.0], **ok)
    out, state = eng.sample_span(cond, mask, y_new, prev, [0, -1], text, grids, [2.0, 0.0], **ok)
    assert state.shape == out.shape == (2, 20, 100) and torch.isfinite(state).all()


# ------------------------------------------------------------------------------------------------ 6. one graph, every slice
G_DURS, G_REFS, G_NTS = [70, 33, 9], [20, 16, 4], [14, 10, 3]
# per call: (start, sway of the call, guidance per item); six steps each, two per call
G_CALLS = [(0, -1.0, [2.0, 0.5, 1.0]), (2, -0.5, [0.5, 3.0, 0.0]), (4, -0.8, [1.5, 2.0, 2.5])]


def graph_chain(model):
    """Three span calls of one shape -- other positions, other grids, other guidance, and for the third a previous state of
    another shape in another row order.  Returns [(out, state)] on the host."""
    cond, text, dur, lens = inputs(G_DURS, G_REFS, G_NTS)
    eng, got, prev = model.transformer.engine(), [], None
    for n, (start, sway, cfgs) in enumerate(G_CALLS):
        if n == 2:                                                      # the same rows inside a larger tensor, permuted
            state, _ = prev
            wide = torch.full((5, 80, 100), NAN, device=DEV)
            wide[[4, 0, 2], :70] = state
            prev = (wide, [4, 0, 2])
        res = model.sample_span(cond, text, dur, lens=lens, steps=6, cfg_strength=cfgs, sway_sampling_coef=sway, seed=3, start=[start] * 3,
                                count=2, prev=prev)
        got.append((res.out.cpu(), res.state.cpu(), eng.graph_stats()))
        prev = (res.state, [0, 1, 2])
    return got


def test_one_graph_serves_every_slice_of_a_shape(monkeypatch):
    rows = {time_rows([(6, c, sway, 3) for c in cfgs], [start] * 3, 2, "euler") for start, sway, cfgs in G_CALLS}
    assert rows == {2}, "the key holds the number of distinct evaluation times: the calls must agree on it"
    monkeypatch.setenv("F5_HIP_GRAPH", "0")
    want = graph_chain(build("sample_b1_nfe16", "f16p"))
    assert want[-1][2] == dict(captures=0, replays=0, eager=3, evictions=0)
    monkeypatch.delenv("F5_HIP_GRAPH")
    got = graph_chain(build("sample_b1_nfe16", "f16p"))
    for n, ((out, state, stats), (want_out, want_state, _)) in enumerate(zip(got, want)):
        assert stats == dict(captures=min(n, 1), replays=max(n - 1, 0), eager=1, evictions=0), f"call {n}"
        assert torch.isfinite(state).all()
        assert torch.equal(state, want_state) and torch.equal(out, want_out), f"call {n} differs from the engine without graphs"
    assert not torch.equal(got[1][1], got[0][1]) and not torch.equal(got[2][1], got[1][1])


# ------------------------------------------------------------------------------------------------ 8. the pool
def test_a_sliced_pool_replayed_from_its_log_and_spans():
    from test_long_form_gpu import tiny_model, tiny_vocoder
    from test_stream_deliver_gpu import KW, SPEED
    from test_stream_pool_gpu import CLIENTS, TEXTS, bank_of
    import emit_oracle as E

    model, voc = tiny_model(False), tiny_vocoder()
    bank = bank_of(model, False)
    own = {"main": {}, "b": dict(nfe_step=3, cfg_strength=0.5), "c": dict(nfe_step=5, cfg_strength=3.0, seed=11)}
    pool = I.open_pool(model, voc, bank, batch_frames=1500, slice_steps=2, **KW)
    clients = {name: pool.connect(name, speed=SPEED, **CLIENTS[name], **own[name]) for name in CLIENTS}
    reqs, packets = {"main": clients["main"].submit(TEXTS["main"])}, {}
    ticks, empty = 0, 0
    while not pool.idle():
        got = pool.step()
        empty += not got
        for r, pk in got:
            packets.setdefault(r.id, []).extend(pk)
        if ticks == 0:
            reqs["b"], reqs["c"] = clients["b"].submit(TEXTS["b"]), clients["c"].submit(TEXTS["c"])
        ticks += 1
    by_id = {r.id: r for r in reqs.values()}
    assert all(r.done and r.under_way == 0 for r in reqs.values())
    stats = pool.stats()
    assert stats["sample_calls"] == stats["ticks"] == len(pool.log) == len(pool.spans) == ticks
    steps_of = {r.id: r.client.sample_kw["steps"] for r in reqs.values()}
    ending = [sum(a + n == steps_of[rid] for (rid, _), (a, n) in zip(items, spans)) for items, spans in zip(pool.log, pool.spans)]
    assert stats["decode_calls"] == stats["emit_launches"] == sum(e > 0 for e in ending) and empty == sum(e == 0 for e in ending)
    assert empty > 0, "no tick ends without a finished row: the case lost its point"
    assert any(0 < e < len(items) for e, items in zip(ending, pool.log)), "no tick ends only some of its rows"
    assert any(len({a for a, _ in spans}) > 1 for spans in pool.spans), "no tick holds rows at different positions"
    # ---- the replay: the same sample_span calls from the log and the spans, the pieces as a tick makes them
    pieces, where = {rid: [] for rid in by_id}, {}
    names = ("steps", "cfg_strength", "sway_sampling_coef", "seed")
    with torch.inference_mode():
        for items, spans in zip(pool.log, pool.spans):
            run = [(by_id[rid], k) for rid, k in items]
            glens = [bank.frames[r.voice] for r, _ in run]
            rows = torch.tensor([r.voice for r, _ in run], device=DEV)
            state, prev_rows = span_prev([where.get(item, (None, -1)) for item in items])
            assert all((a == 0) == (row == -1) for (a, _), row in zip(spans, prev_rows))
            res = model.sample_span(cond=bank.mel[:, :max(glens)].index_select(0, rows), text=[r.plan["texts"][k] for r, k in run],
                                    duration=torch.tensor([r.plan["durations"][k] for r, k in run]), lens=torch.tensor(glens),
                                    start=[a for a, _ in spans], count=2, prev=None if state is None else (state, prev_rows),
                                    **{name: [r.client.sample_kw[name] for r, _ in run] for name in names})
            for b, item in enumerate(items):
                where[item] = (res.state, b)
            ended = [b for b, d in enumerate(res.done) if d]
            assert [a + n == steps_of[rid] for (rid, _), (a, n) in zip(items, spans)] == res.done
            if not ended:
                continue
            pick = torch.tensor(ended, device=DEV)
            wave, wave_lens = voc.decode_ragged(res.out.index_select(0, pick).permute(0, 2, 1), ends=[run[b][0].plan["ends"][run[b][1]] for b in ended],
                                                starts=[bank.samples[run[b][0].voice] // 256 for b in ended])
            wave = I.rescale_to_prompt(wave, bank.rms.index_select(0, rows.index_select(0, pick))[:, None], bank.target_rms)
            for j, b in enumerate(ended):
                assert run[b][1] == len(pieces[run[b][0].id]), "a request's chunks end in order"
                pieces[run[b][0].id].append(wave[j, :wave_lens[j]])
        for name, r in reqs.items():
            c = r.client
            assert len(pieces[r.id]) == len(r.plan["ends"])
            joined = I.wave_join(pieces[r.id], [0] + [c.fade] * (len(pieces[r.id]) - 1))
            want = I.wave_deliver(model.mel_spec, [joined], out_rate=c.out_rate, sample_format=c.sample_format, final=True)[0].cpu().numpy()
            got = np.concatenate(packets[r.id])
            assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(E.as_bytes(got), E.as_bytes(want)), name
