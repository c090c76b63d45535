"""GPU: isolated rows (f5_set_isolated_rows; DiT.set_isolated_rows; open_pool(isolate=True)) -- per-item and sliced solves on packed
rows, in length buckets.

The yardsticks: the two packed per-item update kernels and the pitched staging against their numpy restatements, bit for bit; every
row of an isolated batch on a model WITHOUT attn_mask_enabled against the same item alone -- through an isolated B = 1 call, through
plain sample() at B = 1 on the exact path, and in other batches -- with torch.equal, and against the float64 oracle's solve of the
item alone; a sliced chain against the unsliced isolated solve; one captured graph for calls that differ in N inside a bucket, in
text length and in the number of distinct evaluation times; the refusals; and a pool whose clients get a session's packets.
Every test here needs the setter, which the engine did not have before.  Tiny architectures of the committed fixtures."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import isolate_oracle as ISO  # noqa: E402
import items_oracle as IO  # noqa: E402
from conftest import load_golden, synthetic_weights  # noqa: E402
from gpu_util import DEV, Guarded, _a, _p, _s, k_gemm_plan  # noqa: E402
from test_sample_items_gpu import DURS, NTS, REFS, SETTINGS, build, cached, columns, dev, inputs  # noqa: E402
from test_sample_span_gpu import MASKED, RF_DURS, RF_NTS, RF_REFS, RF_SET, TOL, oracle_items  # noqa: E402

import f5_tts_amd as P  # noqa: E402
from f5_tts_amd import _lib  # noqa: E402
from f5_tts_amd import cfm as CFM_MOD  # noqa: E402
from f5_tts_amd import infer as I  # noqa: E402

FIX = "sample_b1_nfe16"       # attn_mask_enabled = False: a row of a rectangular batch sees its batch


def isolated(fixture, prec, method="euler", bucket=0, arch=None):
    """A fresh model with isolated rows on (never a cached one: the switch is the model's)."""
    meta, _ = load_golden(fixture)
    sd = cached(("sd", fixture), lambda: synthetic_weights(meta))
    tr = P.DiT(**dict(meta["arch"], **(arch or {})), text_num_embeds=meta["nvocab"], mel_dim=100, precision=prec)
    tr.load_state_dict(sd)
    tr.set_isolated_rows(True)
    if bucket:
        tr.set_length_buckets(bucket)
    return P.CFM(transformer=tr, mel_spec_module=P.mel.MelSpec(), odeint_kwargs=dict(method=method)).to(DEV)


# ------------------------------------------------------------------------------------------------ 1. the kernels
K_B, K_N, K_MEL, K_LENS, K_STEPS, K_CFG = 3, 12, 100, [12, 5, 1], [3, 1, 2], [2.0, 0.0, 0.7]


def kernel_case(use_cfg):
    rng = np.random.default_rng(17)
    rs = ISO.row_start(K_LENS, 2 if use_cfg else 1)
    assert rs.tolist() == ([0, 12, 20, 24, 36, 44, 48] if use_cfg else [0, 12, 20, 24])
    y = rng.standard_normal((K_B, K_N, K_MEL)).astype(np.float32)           # the pattern an unwritten frame keeps
    pred = np.full((int(rs[-1]), K_MEL), np.nan, np.float32)                # the alignment rows are never read
    for q in range(len(rs) - 1):
        n = K_LENS[q % K_B]
        pred[rs[q]:rs[q] + n] = rng.standard_normal((n, K_MEL)).astype(np.float32)
    t = np.zeros((K_B, 4), np.float32)
    for b, s in enumerate(K_STEPS):
        t[b, :s + 1] = np.sort(rng.random(s + 1).astype(np.float32))
        t[b, s + 1:] = np.nan                                               # what follows an item's grid is never read
    return y, pred, rs, t


@pytest.mark.parametrize("use_cfg", [1, 0])
@pytest.mark.parametrize("step", [0, 1, 2])
def test_packed_item_update_kernels_are_bit_exact(step, use_cfg):
    lib = _lib.load()
    y, pred, rs, t = kernel_case(use_cfg)
    assert K_B * K_N * K_MEL // 4 > 256, "more than one block"
    held = (dev(rs), dev(K_LENS, torch.int32), dev(t), dev(K_CFG, torch.float32), dev(K_STEPS, torch.int32))   # (kept alive)
    tables = tuple(_p(x) for x in held)
    pred_dev, y_dev = dev(pred), dev(y)
    want = ISO.euler_items_packed(y, pred, rs, K_LENS, t, K_CFG, K_STEPS, step, use_cfg)
    assert not np.isnan(want).any()
    yg, slot = Guarded.like(dev(y)), Guarded((K_B, K_N, K_MEL), torch.float32)
    _lib.check(lib.f5k_euler_cfg_items_packed(_a(yg), _p(pred_dev), K_B, K_N, K_MEL, *tables, 3, step, use_cfg, _a(slot), _s()),
               "f5k_euler_cfg_items_packed")
    assert yg.guards_intact() and slot.guards_intact()
    assert yg.value.cpu().numpy().tobytes() == want.tobytes() and slot.value.cpu().numpy().tobytes() == want.tobytes()
    for b in range(K_B):                                                    # a finished item, and the frames past an item's length
        assert np.array_equal(want[b, K_LENS[b]:], y[b, K_LENS[b]:])
        assert (step < K_STEPS[b]) != np.array_equal(want[b], y[b])
    # ... without a slot
    yg = Guarded.like(dev(y))
    _lib.check(lib.f5k_euler_cfg_items_packed(_a(yg), _p(pred_dev), K_B, K_N, K_MEL, *tables, 3, step, use_cfg, None, _s()),
               "f5k_euler_cfg_items_packed")
    assert yg.guards_intact() and yg.value.cpu().numpy().tobytes() == want.tobytes()
    # the midpoint half step
    mid = Guarded((K_B, K_N, K_MEL), torch.float32)
    _lib.check(lib.f5k_midpoint_half_cfg_items_packed(_p(y_dev), _p(pred_dev), K_B, K_N, K_MEL, *tables, 3, step, use_cfg, _a(mid), _s()),
               "f5k_midpoint_half_cfg_items_packed")
    assert mid.guards_intact()
    assert mid.value.cpu().numpy().tobytes() == ISO.midpoint_half_items_packed(y, pred, rs, K_LENS, t, K_CFG, K_STEPS, step, use_cfg).tobytes()
    assert torch.equal(y_dev.cpu(), torch.from_numpy(y)), "the half step does not write y"
    # refusals: no tables, a step past every grid, no y_mid
    args = (_p(y_dev), _p(pred_dev), K_B, K_N, K_MEL)
    assert lib.f5k_euler_cfg_items_packed(*args, None, tables[1], *tables[2:], 3, 0, 1, None, _s()) == -1 and b"row_start" in lib.f5_last_error()
    assert lib.f5k_euler_cfg_items_packed(*args, *tables, 3, 3, 1, None, _s()) == -1
    assert lib.f5k_midpoint_half_cfg_items_packed(*args, *tables, 3, 0, 1, None, _s()) == -1


@pytest.mark.parametrize("prev_N", [7, 12, 15])
def test_pitched_span_stage_is_bit_exact(prev_N):
    lib = _lib.load()
    B, N, pitch, mel, prev_B, rows = 3, 12, 16, 100, 3, [2, -1, 0]
    rng = np.random.default_rng(prev_N)
    prev = rng.standard_normal((prev_B, prev_N, mel)).astype(np.float32)
    prev[1] = np.nan                                                        # a row nobody continues
    y_new = np.full((B, N, mel), np.nan, np.float32)                        # the rows of continuing items are not read
    y_new[1] = rng.standard_normal((N, mel)).astype(np.float32)
    y0 = rng.standard_normal((B, pitch, mel)).astype(np.float32)
    y, prev_dev, new_dev, rows_dev = Guarded.like(dev(y0)), dev(prev), dev(y_new), dev(rows, torch.int32)
    _lib.check(lib.f5k_span_stage_pitched(_a(y), pitch, _p(prev_dev), prev_B, prev_N, _p(new_dev), _p(rows_dev), _lib.int_array(rows), B, N, mel,
                                          _s()), "f5k_span_stage_pitched")
    want = ISO.span_stage_pitched(y0, prev, y_new, rows, N)
    assert not np.isnan(want).any() and np.array_equal(want[:, N:], y0[:, N:])
    assert y.guards_intact() and y.value.cpu().numpy().tobytes() == want.tobytes()
    # pitch == N is f5k_span_stage; a pitch below N is refused and writes nothing
    a, b = Guarded((B, N, mel), torch.float32), Guarded((B, N, mel), torch.float32)
    _lib.check(lib.f5k_span_stage_pitched(_a(a), N, _p(prev_dev), prev_B, prev_N, _p(new_dev), _p(rows_dev), _lib.int_array(rows), B, N, mel, _s()),
               "f5k_span_stage_pitched")
    _lib.check(lib.f5k_span_stage(_a(b), _p(prev_dev), prev_B, prev_N, _p(new_dev), _p(rows_dev), _lib.int_array(rows), B, N, mel, _s()),
               "f5k_span_stage")
    assert a.guards_intact() and torch.equal(a.bits, b.bits) and a.value.cpu().numpy().tobytes() == want[:, :N].tobytes()
    c = Guarded((B, N, mel), torch.float32)
    assert lib.f5k_span_stage_pitched(_a(c), N - 1, _p(prev_dev), prev_B, prev_N, _p(new_dev), _p(rows_dev), _lib.int_array(rows), B, N, mel,
                                      _s()) == -1 and b"pitch" in lib.f5_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(c.value).all()


# ------------------------------------------------------------------------------------------------ 2. isolation
def time_rows_of(settings, method):
    grids = [g.tolist() for g in CFM_MOD.item_time_grids([s[0] for s in settings], [s[2] for s in settings])]
    return len(IO.item_time_rows(grids, [s[0] for s in settings], method)[0])


def pow2(n):
    return 1 << (n - 1).bit_length()


def single(i, durs=DURS, refs=REFS, nts=NTS):
    """Item i of inputs(durs, refs, nts) as a batch of its own: its prompt and its text at their own lengths."""
    cond, text, dur, lens = inputs(durs, refs, nts)
    return cond[i:i + 1, :refs[i]], text[i:i + 1, :nts[i]], dur[i:i + 1], lens[i:i + 1]


@pytest.mark.parametrize("prec", ["f32", "f16p"])
@pytest.mark.parametrize("method", ["euler", "midpoint"])
def test_every_row_is_the_item_alone_bit_for_bit(method, prec):
    """Section 6m's mixed batch on a model whose rectangular batch lets a short row attend over the padding.  The chain behind the
    middle comparison -- a uniform sample_items is sample(), the packed (bucket) body is the exact body -- is pinned elsewhere."""
    meta, _ = load_golden(FIX)
    assert not meta["arch"]["attn_mask_enabled"]
    # (the time path's f32 GEMMs run at other row counts in the three calls: they must plan them alike, as test_sample_items_gpu.py checks)
    evals = 2 if method == "midpoint" else 1
    D, modN = meta["arch"]["dim"], (6 * meta["arch"]["depth"] + 2) * meta["arch"]["dim"]
    FIFTH = (3, 1.5, -0.7, 21)
    counts = {pow2(time_rows_of(SETTINGS, method)), pow2(time_rows_of(SETTINGS + [FIFTH], method))}
    counts |= {pow2(s[0] * evals) for s in SETTINGS} | {s[0] * evals for s in SETTINGS}
    for n, k in ((D, 256), (D, D), (modN, D)):
        tiles = {m: [(fam, tile) for fam, tile, _, _ in k_gemm_plan(4, m, n, k)] for m in sorted(counts)}
        assert len({str(t) for t in tiles.values()}) == 1, f"the time path's [{n} x {k}] GEMM plans its row counts differently: {tiles}"
    model = isolated(FIX, prec, method)
    cond, text, dur, lens = inputs(DURS, REFS, NTS)
    out, traj = (t.cpu() for t in model.sample_items(cond, text, dur, lens=lens, **columns(SETTINGS)))
    assert traj.shape == (5, 4, 129, 100) and torch.isfinite(traj).all()
    rect_out, _ = build(FIX, prec, method).sample_items(cond, text, dur, lens=lens, **columns(SETTINGS))
    assert not torch.equal(rect_out.cpu()[1, :17], out[1, :17]), "the rectangular batch does depend on the batch: the case has a point"
    for i, (steps, cfg, sway, seed) in enumerate(SETTINGS):
        n = DURS[i]
        c1, t1, d1, l1 = single(i)
        # (a) the item through an isolated B = 1 call
        a_out, a_traj = (t.cpu() for t in model.sample_items(c1, t1, d1, lens=l1, steps=[steps], cfg_strength=[cfg], sway_sampling_coef=[sway], seed=[seed]))
        assert a_traj.shape == (steps + 1, 1, n, 100)
        assert torch.equal(traj[:steps + 1, i, :n], a_traj[:, 0]) and torch.equal(out[i, :n], a_out[0]), f"item {i}: isolated B = 1"
        # (b) the item through plain sample() at B = 1 on the exact path
        b_out, b_traj = (t.cpu() for t in model.sample(c1, t1, d1, lens=l1, steps=steps, cfg_strength=cfg, sway_sampling_coef=sway, seed=seed))
        assert torch.equal(traj[:steps + 1, i, :n], b_traj[:, 0]) and torch.equal(out[i, :n], b_out[0]), f"item {i}: sample() at B = 1"
        # frames past the item's own length keep their staged value (the zero padding of its noise; the mask is false there)
        assert (traj[:, i, n:] == 0).all() and (out[i, n:] == 0).all(), f"item {i}: frames past its length"
        for later in range(steps + 1, 5):
            assert torch.equal(traj[later, i], traj[steps, i]), f"item {i}: a finished item keeps its state"
    # (c) another row order, and a fifth, longer item beside them
    perm = [2, 0, 3, 1]
    p_out, p_traj = (t.cpu() for t in model.sample_items(cond[perm], text[perm], dur[perm], lens=lens[perm], **columns([SETTINGS[i] for i in perm])))
    for row, i in enumerate(perm):
        assert torch.equal(p_traj[:, row, :DURS[i]], traj[:, i, :DURS[i]]) and torch.equal(p_out[row, :DURS[i]], out[i, :DURS[i]]), f"item {i} in row {row}"
    cond5, text5, dur5, lens5 = inputs(DURS + [150], REFS + [25], NTS + [11])
    cond5[:4, :max(REFS)], text5[:4, :max(NTS)] = cond, text                # the four items as they were, a new one behind them
    w_out, w_traj = (t.cpu() for t in model.sample_items(cond5, text5, dur5, lens=lens5, **columns(SETTINGS + [FIFTH])))
    assert w_traj.shape == (5, 5, 150, 100)
    for i in range(4):
        assert torch.equal(w_traj[:, i, :DURS[i]], traj[:, i, :DURS[i]]) and torch.equal(w_out[i, :DURS[i]], out[i, :DURS[i]]), f"item {i} beside a fifth"


# ------------------------------------------------------------------------------------------------ 3. against float64
@pytest.mark.parametrize("prec", ["f32", "f16p", "f16", "bf16"])
def test_isolated_rows_against_the_oracle_item_by_item(prec):
    """test_sample_span_gpu.py's reference -- the float64 oracle's solve of every item of RF_SET alone -- and its bars.  At B = 1
    masked and unmasked attention coincide, so the reference serves the same weights WITHOUT attn_mask_enabled, where only an
    isolated row is the item alone."""
    model = isolated(MASKED, prec, arch=dict(attn_mask_enabled=False))
    cond, text, dur, lens = inputs(RF_DURS, RF_REFS, RF_NTS)
    out, traj = (t.cpu() for t in model.sample_items(cond, text, dur, lens=lens, **columns(RF_SET)))
    for i, (want_out, want_state) in enumerate(oracle_items()):
        n, s = RF_DURS[i], RF_SET[i][0]
        e_out = (out[i, :n] - want_out).abs().max().item()
        e_state = (traj[s, i, :n] - want_state).abs().max().item()
        print(f"[isolated {prec}] item {i} {RF_SET[i]}: state Linf {e_state:.3e} out Linf {e_out:.3e}")
        assert e_out < TOL[prec] and e_state < TOL[prec], f"item {i}"


# ------------------------------------------------------------------------------------------------ 4. slices
@pytest.mark.parametrize("bucket", [0, 8])
@pytest.mark.parametrize("method", ["euler", "midpoint"])
def test_a_sliced_chain_is_the_unsliced_isolated_solve(method, bucket):
    """Three slices: the 129-frame item (2 steps) ends in the first and leaves; the 40-frame item joins in the second, in another
    row order, and N shrinks to 66; the third ends the rest.  Inside its frames every item is its row of the unsliced isolated
    solve of all four."""
    model = isolated(FIX, "f16p", method, bucket)
    cond, text, dur, lens = inputs(RF_DURS, RF_REFS, RF_NTS)
    want_out, want_traj = (t.cpu() for t in model.sample_items(cond, text, dur, lens=lens, **columns(RF_SET)))

    def span(keep, start, count, prev):
        return model.sample_span(cond[keep], text[keep], dur[keep], lens=lens[keep], start=start, count=count, prev=prev,
                                 **columns([RF_SET[i] for i in keep]))

    def check(res, keep, made):
        for row, (i, m) in enumerate(zip(keep, made)):
            n = RF_DURS[i]
            assert torch.equal(res.state.cpu()[row, :n], want_traj[m, i, :n]), f"item {i} after {m} steps"
            if m == RF_SET[i][0]:
                assert res.done[row] and torch.equal(res.out.cpu()[row, :n], want_out[i, :n]), f"item {i}: out"

    one = span([0, 1, 2], [0, 0, 0], 2, None)
    assert one.done == [False, True, False] and one.state.shape == (3, 129, 100)
    check(one, [0, 1, 2], [2, 2, 2])
    two = span([2, 3, 0], [2, 0, 2], 1, (one.state, [2, -1, 0]))
    assert two.done == [False, False, False] and two.state.shape == (3, 66, 100)
    check(two, [2, 3, 0], [3, 1, 3])
    three = span([0, 3, 2], [3, 1, 3], 2, (two.state, [2, 1, 0]))
    assert three.done == [True, True, True]
    check(three, [0, 3, 2], [4, 3, 4])


# ------------------------------------------------------------------------------------------------ 5. graphs
G_REFS = [10, 8, 4]
# per call: durations (one bucket of 8: ceiling 48), text lengths (the first call has the longest), (steps, cfg, sway, seed) per item
G_CALLS = [([41, 30, 9], [14, 10, 3], [(3, 2.0, -1.0, 3), (3, 0.5, -0.5, 5), (3, 1.0, None, 7)]),       # three grids: 7 time rows
           ([44, 33, 12], [9, 12, 2], [(3, 0.5, -0.8, 11), (3, 2.0, -0.8, 13), (3, 3.0, -0.2, 17)]),    # two share a grid: 5
           ([47, 20, 47], [5, 3, 8], [(3, 1.5, None, 19), (3, 0.0, -1.0, 23), (2, 2.5, -0.3, 29)]),     # an item of two steps: 6
           ([48, 48, 17], [11, 6, 1], [(3, 2.0, -0.6, 31), (3, 1.0, -0.9, 37), (3, 0.0, -0.1, 41)])]    # 7


def graph_calls(model):
    got = []
    eng = model.transformer.engine()
    for durs, nts, settings in G_CALLS:
        cond, text, dur, lens = inputs(durs, G_REFS, nts)
        out, traj = model.sample_items(cond, text, dur, lens=lens, **columns(settings))
        got.append((out.cpu(), traj.cpu(), eng.graph_stats()))
    return got


def test_one_graph_serves_a_bucket_every_text_length_and_a_range_of_time_rows(monkeypatch):
    rows = [time_rows_of(settings, "euler") for _, _, settings in G_CALLS]
    assert rows == [7, 5, 6, 7] and {pow2(u) for u in rows} == {8}, rows
    assert {-(-max(durs) // 8) * 8 for durs, _, _ in G_CALLS} == {48} and len({max(durs) for durs, _, _ in G_CALLS}) == 4
    assert max(G_CALLS[0][1]) == max(max(nts) for _, nts, _ in G_CALLS) and len({max(nts) for _, nts, _ in G_CALLS}) == 4
    monkeypatch.setenv("F5_HIP_GRAPH", "0")
    want = graph_calls(isolated(FIX, "f16p", bucket=8))
    assert want[-1][2] == dict(captures=0, replays=0, eager=4, evictions=0)
    monkeypatch.delenv("F5_HIP_GRAPH")
    got = graph_calls(isolated(FIX, "f16p", bucket=8))
    for n, ((out, traj, stats), (want_out, want_traj, _)) in enumerate(zip(got, want)):
        assert stats == dict(captures=min(n, 1), replays=max(n - 1, 0), eager=1, evictions=0), f"call {n}: {stats}"
        assert torch.isfinite(traj).all()
        assert torch.equal(traj, want_traj) and torch.equal(out, want_out), f"call {n} differs from the engine without graphs"
    # and the bucketed rows are the exact ones
    exact = isolated(FIX, "f16p")
    durs, nts, settings = G_CALLS[2]
    cond, text, dur, lens = inputs(durs, G_REFS, nts)
    e_out, e_traj = exact.sample_items(cond, text, dur, lens=lens, **columns(settings))
    assert torch.equal(e_traj.cpu(), got[2][1]) and torch.equal(e_out.cpu(), got[2][0])
    eng = exact.transformer.engine()
    for n in (15, 65):
        with pytest.raises(_lib.F5Error, match="f5_set_graph_capacity"):
            eng.set_graph_capacity(n)
    eng.set_graph_capacity(64)


# ------------------------------------------------------------------------------------------------ 6. refusals
def refused(model, match):
    eng = model.transformer.engine()
    cond, text, dur, lens = inputs([40, 12], [6, 4], [5, 3])
    eng.graph_stats(reset=True)
    with pytest.raises(_lib.F5Error, match=match):
        model.sample_items(cond, text, dur, lens=lens, steps=[2, 1], cfg_strength=[2.0, 0.5], sway_sampling_coef=-1.0, seed=3)
    with pytest.raises(_lib.F5Error, match=match):
        model.sample_span(cond, text, dur, lens=lens, steps=[2, 1], cfg_strength=[2.0, 0.5], sway_sampling_coef=-1.0, seed=3, start=[0, 0], count=2)
    assert eng.graph_stats() == dict(captures=0, replays=0, eager=0, evictions=0), "a refused call runs no body"
    return eng


def test_a_call_that_cannot_be_isolated_is_refused_with_its_reason(monkeypatch):
    # the UNetT: the model refuses the switch; an engine that is given it refuses the call, and runs again without it
    unett = build("sample_unett_b2", "f16x3")
    with pytest.raises(NotImplementedError, match="isolated rows"):
        unett.transformer.set_isolated_rows(True)
    unett.transformer.engine().set_isolated_rows(True)
    eng = refused(unett, "f5_sample_(items|span): isolated rows.*UNetT")
    eng.set_isolated_rows(False)
    cond, text, dur, lens = inputs([40, 12], [6, 4], [5, 3])
    out, _ = unett.sample_items(cond, text, dur, lens=lens, steps=[2, 1], cfg_strength=[2.0, 0.5], sway_sampling_coef=-1.0, seed=3)
    assert torch.isfinite(out).all()
    # text_embedding_average_upsampling
    meta, _ = load_golden(FIX)
    arch = dict(meta["arch"], text_mask_padding=True, text_embedding_average_upsampling=True)
    tr = P.DiT(**arch, text_num_embeds=meta["nvocab"], mel_dim=100, precision="f32").init_synthetic(seed=1)
    tr.set_isolated_rows(True)
    refused(P.CFM(transformer=tr, mel_spec_module=P.mel.MelSpec()).to(DEV), "isolated rows.*text_embedding_average_upsampling")
    # a bucket ceiling past max_pos: 40 frames fit 64 positions, the ceiling of 64 (+ 1) does not
    tr = P.DiT(**meta["arch"], text_num_embeds=meta["nvocab"], mel_dim=100, precision="f32", max_pos=64).init_synthetic(seed=1)
    tr.set_isolated_rows(True)
    tr.set_length_buckets(64)
    small = P.CFM(transformer=tr, mel_spec_module=P.mel.MelSpec()).to(DEV)
    refused(small, "isolated rows: N=40 is planned at 64 frames.*max_pos = 64")
    tr.set_length_buckets(0)
    cond, text, dur, lens = inputs([40, 12], [6, 4], [5, 3])
    out, _ = small.sample_items(cond, text, dur, lens=lens, steps=[2, 1], cfg_strength=[2.0, 0.5], sway_sampling_coef=-1.0, seed=3)
    assert torch.isfinite(out).all(), "at its exact N the call runs"
    # F5_SPLIT_CFG=1 (read when the engine is created); F5_PACK_ROWS=0 does not turn isolation off
    monkeypatch.setenv("F5_SPLIT_CFG", "1")
    refused(isolated(FIX, "f32"), "isolated rows.*F5_SPLIT_CFG")
    monkeypatch.delenv("F5_SPLIT_CFG")
    monkeypatch.setenv("F5_PACK_ROWS", "0")
    unpacked = isolated(FIX, "f32")
    cond, text, dur, lens = inputs(DURS, REFS, NTS)
    out, _ = unpacked.sample_items(cond, text, dur, lens=lens, **columns(SETTINGS))
    monkeypatch.delenv("F5_PACK_ROWS")
    want, _ = isolated(FIX, "f32").sample_items(cond, text, dur, lens=lens, **columns(SETTINGS))
    assert torch.equal(out, want)


# ------------------------------------------------------------------------------------------------ 7. the switch off
def test_with_the_switch_off_nothing_moves():
    cond, text, dur, lens = inputs(DURS, REFS, NTS)
    never = build(FIX, "f16p")
    toggled = build(FIX, "f16p")
    toggled.transformer.set_isolated_rows(True)
    toggled.transformer.engine()
    toggled.transformer.set_isolated_rows(False)
    for model in (never, toggled):
        model.runs = [tuple(t.cpu() for t in model.sample_items(cond, text, dur, lens=lens, **columns(SETTINGS))) for _ in range(3)]
    assert never.transformer.graph_stats() == toggled.transformer.graph_stats() == dict(captures=1, replays=1, eager=1, evictions=0)
    for a, b in zip(never.runs, toggled.runs):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    u_out, u_traj = toggled.sample(cond, text, dur, lens=lens, steps=4, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=3)
    toggled.transformer.set_isolated_rows(True)
    on_out, on_traj = toggled.sample(cond, text, dur, lens=lens, steps=4, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=3)
    assert torch.equal(on_out, u_out) and torch.equal(on_traj, u_traj), "sample() does not hear of the switch"
    iso_out, _ = toggled.sample_items(cond, text, dur, lens=lens, **columns(SETTINGS))
    stats = toggled.transformer.graph_stats()
    assert stats["eager"] == 3 and stats["captures"] == 2, "an isolated call has a key of its own: the rectangular graph is not replayed for it"
    assert not torch.equal(iso_out.cpu()[1, :17], never.runs[0][0][1, :17])


# ------------------------------------------------------------------------------------------------ 8. the pool
def test_an_isolated_pools_packets_are_a_sessions():
    """Three clients of unequal chunk lengths on a model without attn_mask_enabled, solved in slices of two of four steps: every
    request's packets, concatenated, are byte for byte those of the same request through a StreamSession, which runs every chunk
    alone (where a packet ends depends on which chunks a tick delivered together, not on the audio: StreamPool promises the
    concatenation).  Without isolate they are not."""
    from test_long_form_gpu import tiny_vocoder
    from test_stream_deliver_gpu import KW, SPEED
    from test_stream_pool_gpu import CLIENTS, TEXTS, voices
    import emit_oracle as E

    def same_stream(got, want):
        a, b = np.concatenate(got), np.concatenate(want)
        return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(E.as_bytes(a), E.as_bytes(b))

    kw = dict(KW, nfe_step=4)
    tr = P.DiT(**dict(P.config.F5TTS_TINY, attn_mask_enabled=False), text_num_embeds=257, mel_dim=100, precision="f32").init_synthetic(seed=2)
    model, voc = P.CFM(transformer=tr).to(DEV), tiny_vocoder()
    bank = I.prepare_voices(model, voices())
    want = {}
    for name in CLIENTS:
        session = I.open_stream(model, voc, (bank, name), speed=SPEED, **CLIENTS[name], **kw)
        want[name] = [p for p, _ in session.stream(TEXTS[name])]

    def serve(**pool_kw):
        pool = I.open_pool(model, voc, bank, batch_frames=1500, slice_steps=2, **pool_kw, **kw)
        clients = {name: pool.connect(name, speed=SPEED, **CLIENTS[name]) for name in CLIENTS}
        reqs, packets, first = {"main": clients["main"].submit(TEXTS["main"])}, {}, True
        while not pool.idle():
            for r, pk in pool.step():
                packets.setdefault(r.id, []).extend(pk)
            if first:
                reqs["b"], reqs["c"] = clients["b"].submit(TEXTS["b"]), clients["c"].submit(TEXTS["c"])
                first = False
        assert all(r.done for r in reqs.values())
        return pool, {name: packets[r.id] for name, r in reqs.items()}

    pool, got = serve(isolate=True)
    assert pool.stats()["isolated"] is True and tr.isolated_rows and tr.graph_capacity == 64
    assert any(len(tick) > 1 for tick in pool.log), "no tick shares rows: the case lost its point"
    assert any(len({a for a, _ in spans}) > 1 for spans in pool.spans), "no tick holds rows at different positions"
    for name in CLIENTS:
        assert same_stream(got[name], want[name]), f"client {name}: not the session's bytes"
    tr.set_isolated_rows(False)
    _, plain = serve()
    differs = [name for name in CLIENTS if not same_stream(plain[name], want[name])]
    assert differs, "without isolate the rectangular ticks gave a session's bits too: the case shows nothing"
