"""GPU: per-item sampler settings in one ragged batch (f5_sample_items; CFM.sample_items; a pool whose clients differ).

Batch rows never interact -- attention, convolutions and masks are per row -- so the reference value of item i of a mixed batch is
row i of the whole batch run with item i's settings: the CPU oracle in a loop over the distinct settings, and, bit for bit, the
engine's own sample().  Tiny architectures of the committed fixtures, a few steps."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import items_oracle as IO  # noqa: E402
from conftest import load_golden, synthetic_weights  # noqa: E402
from gpu_util import DEV, Guarded, _a, _p, _s, k_gemm_plan  # noqa: E402
from oracle import f5_oracle as O  # noqa: E402

import f5_tts_amd as P  # noqa: E402
from f5_tts_amd import _lib  # noqa: E402
from f5_tts_amd import cfm as CFM_MOD  # noqa: E402
from f5_tts_amd import infer as I  # noqa: E402

# test_sample_gpu.py's own bars (the arithmetic is the same)
TOL = {"f32": 1e-3, "f16p": 1e-3, "f16x3": 1e-3, "bf16": 3e-2, "f16": 4e-3}
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def build(fixture, prec, method="euler"):
    meta, _ = load_golden(fixture)
    sd = cached(("sd", fixture), lambda: synthetic_weights(meta))
    cls = P.UNetT if meta.get("backbone", "DiT") == "UNetT" else P.DiT
    tr = cls(**meta["arch"], text_num_embeds=meta["nvocab"], mel_dim=100, precision=prec)
    tr.load_state_dict(sd)
    return P.CFM(transformer=tr, mel_spec_module=P.mel.MelSpec(), odeint_kwargs=dict(method=method)).to(DEV)


def inputs(durs, refs, nts, nv=40):
    """cond [B, max ref, 100] (zero behind each prompt), text [B, max nt] (-1 padded), durations, prompt lengths."""
    B = len(durs)
    g = torch.Generator().manual_seed(sum(durs) + 7 * B)
    cond = torch.zeros(B, max(refs), 100)
    text = torch.full((B, max(nts)), -1, dtype=torch.long)
    for i in range(B):
        cond[i, :refs[i]] = torch.randn(refs[i], 100, generator=g)
        text[i, :nts[i]] = torch.randint(0, nv - 1, (nts[i],), generator=g)
    return cond, text, torch.tensor(durs), torch.tensor(refs)


def columns(settings):
    steps, cfgs, sways, seeds = (list(c) for c in zip(*settings))
    return dict(steps=steps, cfg_strength=cfgs, sway_sampling_coef=sways, seed=seeds)


# ------------------------------------------------------------------------------------------------ 1. uniform == sample()
@pytest.mark.parametrize("prec", ["f32", "f16p"])
@pytest.mark.parametrize("method", ["euler", "midpoint"])
def test_uniform_batch_equals_sample_bit_for_bit(method, prec):
    cond, text, dur, lens = inputs([70, 33, 9], [20, 16, 4], [14, 10, 3])
    kw = dict(steps=3, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=3)
    model = build("sample_b1_nfe16", prec, method)
    want_out, want_traj = model.sample(cond, text, dur, lens=lens, **kw)
    eng = model.transformer.engine()
    eng.graph_stats(reset=True)
    for rep in range(3):   # eager, then captured, then replayed
        out, traj = model.sample_items(cond, text, dur, lens=lens, **kw)
        assert traj.shape == want_traj.shape
        assert torch.equal(traj, want_traj) and torch.equal(out, want_out), f"{method} {prec}: run {rep} differs from sample()"
    assert eng.graph_stats() == dict(captures=1, replays=1, eager=1, evictions=0)
    # sequences of equal entries are the same call
    out, traj = model.sample_items(cond, text, dur, lens=lens, steps=[3] * 3, cfg_strength=[2.0] * 3, sway_sampling_coef=[-1.0] * 3, seed=[3] * 3)
    assert torch.equal(traj, want_traj) and torch.equal(out, want_out) and eng.graph_stats()["replays"] == 2


# ------------------------------------------------------------------------------------------------ 2 - 4. a mixed batch
DURS, REFS, NTS = [129, 17, 66, 40], [30, 6, 20, 12], [12, 5, 9, 7]     # 129 crosses a 128-row tile and a 64-key tile
# (steps, cfg, sway, seed); the last item's seed would be None in service: it has one here so that the case is deterministic
SETTINGS = [(4, 2.0, -1.0, 3), (2, 0.0, None, 5), (4, 0.5, -1.0, 3), (3, 2.0, -0.5, 9)]


def oracle_rows(fixture="sample_b1_nfe16", durs=DURS, refs=REFS, nts=NTS, settings=SETTINGS):
    """want[i] = (out row i, traj[:, i]) of the oracle on the WHOLE batch with item i's settings and the mixed call's noise.
    Computed once per distinct setting, never modified."""
    def make():
        meta, _ = load_golden(fixture)
        sd = cached(("sd", fixture), lambda: synthetic_weights(meta))
        cond, text, dur, lens = inputs(durs, refs, nts)
        y0 = CFM_MOD.item_noise(durs, [s[3] for s in settings], 100)
        runs, want = {}, []
        for i, (steps, cfg, sway, _seed) in enumerate(settings):
            if (steps, cfg, sway) not in runs:
                runs[(steps, cfg, sway)] = O.sample(sd, meta["arch"], cond, text, dur, lens=lens, steps=steps, cfg_strength=cfg,
                                                    sway_sampling_coef=sway, y0=y0, backbone=meta.get("backbone", "DiT"))
            out, traj = runs[(steps, cfg, sway)]
            want.append((out[i], traj[:, i]))
        return want
    return cached(("oracle rows", fixture, tuple(durs)), make)


def mixed_run(prec, method="euler"):
    def make():
        cond, text, dur, lens = inputs(DURS, REFS, NTS)
        model = build("sample_b1_nfe16", prec, method)
        out, traj = model.sample_items(cond, text, dur, lens=lens, **columns(SETTINGS))
        return model, out.cpu(), traj.cpu()
    return cached(("mixed run", prec, method), make)


@pytest.mark.parametrize("prec", ["f32", "f16p", "f16", "bf16"])
def test_mixed_batch_against_the_oracle(prec):
    _, out, traj = mixed_run(prec)
    assert traj.shape == (5, 4, 129, 100) and out.shape == (4, 129, 100)
    for i, (want_out, want_traj) in enumerate(oracle_rows()):
        s = SETTINGS[i][0]
        e_traj = (traj[:s + 1, i] - want_traj).abs().max().item()
        e_out = (out[i] - want_out).abs().max().item()
        print(f"[items {prec}] item {i} {SETTINGS[i]}: traj Linf {e_traj:.3e} out Linf {e_out:.3e}")
        assert e_traj < TOL[prec] and e_out < TOL[prec], f"item {i}"


@pytest.mark.parametrize("prec", ["f32", "f16p"])
@pytest.mark.parametrize("method", ["euler", "midpoint"])
def test_mixed_batch_equals_the_uniform_runs_bit_for_bit(method, prec):
    """Row i of the mixed call against row i of sample(whole batch, settings_i): the same kernels on the same rows, provided the
    time-path GEMMs take the same tile for the mixed call's rows as for a uniform call's."""
    meta, _ = load_golden("sample_b1_nfe16")
    D, modN = meta["arch"]["dim"], (6 * meta["arch"]["depth"] + 2) * meta["arch"]["dim"]
    grids = [g.tolist() for g in CFM_MOD.item_time_grids([s[0] for s in SETTINGS], [s[2] for s in SETTINGS])]
    evals = 2 if method == "midpoint" else 1
    U = len(IO.item_time_rows(grids, [s[0] for s in SETTINGS], method)[0])
    assert U == {"euler": 7, "midpoint": 16}[method], "one row per distinct evaluation time: t = 0 is shared, items 0 and 2 share a grid"
    for n, k in ((D, 256), (D, D), (modN, D)):     # the three GEMMs of the time path, f32
        tiles = {m: [(fam, tile) for fam, tile, _, _ in k_gemm_plan(4, m, n, k)] for m in (U, 4 * evals, 3 * evals)}
        assert len({str(t) for t in tiles.values()}) == 1, f"the time path's [{n} x {k}] GEMM plans its row counts differently: {tiles}"
    model, out, traj = mixed_run(prec, method)
    cond, text, dur, lens = inputs(DURS, REFS, NTS)
    checked = 0
    for i, (steps, cfg, sway, seed) in enumerate(SETTINGS):
        if cfg < 1e-5:
            continue   # (its uniform run has half the rows: the oracle test holds it)
        u_out, u_traj = model.sample(cond, text, dur, lens=lens, steps=steps, cfg_strength=cfg, sway_sampling_coef=sway, seed=seed)
        assert torch.equal(traj[:steps + 1, i], u_traj.cpu()[:, i]) and torch.equal(out[i], u_out.cpu()[i]), f"item {i} {SETTINGS[i]}"
        checked += 1
    assert checked == 3


def test_a_finished_item_keeps_its_final_state():
    _, out, traj = mixed_run("f32")
    cond, _, _, lens = inputs(DURS, REFS, NTS)
    N = traj.shape[2]
    cond = torch.nn.functional.pad(cond, (0, 0, 0, N - cond.shape[1]))
    mask = (torch.arange(N)[None, :] < lens[:, None])[..., None]
    for i, (s, *_rest) in enumerate(SETTINGS):
        for later in range(s + 1, traj.shape[0]):
            assert torch.equal(traj[later, i], traj[s, i]), f"item {i}: slot {later} differs from its final state (slot {s})"
        assert torch.equal(out[i], torch.where(mask[i], cond[i], traj[s, i])), f"item {i}: out"
    assert not torch.equal(traj[2, 1], traj[1, 1]) and not torch.equal(traj[4, 0], traj[3, 0]), "the live steps do move the state"


# ------------------------------------------------------------------------------------------------ 5. one graph, many settings
CALLS = [[(3, 2.0, -1.0, 3), (2, 0.5, None, 5), (3, 1.0, -0.5, 7)],
         [(3, 0.5, -0.8, 11), (2, 2.0, -0.2, 13), (3, 3.0, None, 17)],
         [(3, 1.5, None, 19), (2, 0.0, -1.0, 23), (3, 2.5, -0.3, 29)],
         [(3, 2.0, -0.6, 31), (2, 1.0, -0.9, 37), (3, 0.0, -0.1, 41)]]


def test_one_graph_serves_every_setting_of_a_shape(monkeypatch):
    rows = set()
    for call in CALLS:   # the key holds the number of distinct evaluation times: the calls must agree on it, or they are not one shape
        grids = [g.tolist() for g in CFM_MOD.item_time_grids([s[0] for s in call], [s[2] for s in call])]
        rows.add(len(IO.item_time_rows(grids, [s[0] for s in call], "euler")[0]))
    assert len(rows) == 1, rows
    cond, text, dur, lens = inputs([70, 33, 9], [20, 16, 4], [14, 10, 3])
    monkeypatch.setenv("F5_HIP_GRAPH", "0")
    plain = build("sample_b1_nfe16", "f16p")
    want = [tuple(t.cpu() for t in plain.sample_items(cond, text, dur, lens=lens, **columns(call))) for call in CALLS]
    assert plain.transformer.engine().graph_stats() == dict(captures=0, replays=0, eager=len(CALLS), evictions=0)
    monkeypatch.delenv("F5_HIP_GRAPH")
    model = build("sample_b1_nfe16", "f16p")
    eng = model.transformer.engine()
    for n, call in enumerate(CALLS):
        out, traj = model.sample_items(cond, text, dur, lens=lens, **columns(call))
        assert eng.graph_stats() == dict(captures=min(n, 1), replays=max(n - 1, 0), eager=1, evictions=0), f"call {n}"
        assert torch.equal(traj.cpu(), want[n][1]) and torch.equal(out.cpu(), want[n][0]), f"call {n} differs from the eager engine"


# ------------------------------------------------------------------------------------------------ 6. the kernels
def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if dtype is None else torch.tensor(a, dtype=dtype, device=DEV)


K_B, K_N, K_MEL, K_STEPS, K_CFG = 3, 5, 100, [3, 1, 2], [2.0, 0.0, 0.5]


def kernel_case():
    rng = np.random.default_rng(5)
    y = rng.standard_normal((K_B, K_N, K_MEL)).astype(np.float32)
    pred = rng.standard_normal((2, K_B, K_N, K_MEL)).astype(np.float32)
    t = np.zeros((K_B, 4), np.float32)
    for b, s in enumerate(K_STEPS):
        t[b, :s + 1] = np.sort(rng.random(s + 1).astype(np.float32))
        t[b, s + 1:] = np.nan                                          # what follows an item's grid is never read
    return y, pred, t


@pytest.mark.parametrize("use_cfg", [1, 0])
@pytest.mark.parametrize("step", [0, 1, 2])
def test_item_update_kernels_are_bit_exact(step, use_cfg):
    lib = _lib.load()
    y, pred, t = kernel_case()
    assert K_B * K_N * K_MEL // 4 > 256, "more than one block"
    held = (dev(t), dev(K_CFG, torch.float32), dev(K_STEPS, torch.int32))     # (kept alive: the calls take their addresses)
    tables = tuple(_p(x) for x in held)
    pred_dev, y_dev = dev(pred), dev(y)
    # Euler: in place, and into the trajectory slot
    yg, slot = Guarded.like(dev(y)), Guarded((K_B, K_N, K_MEL), torch.float32)
    _lib.check(lib.f5k_euler_cfg_items(_a(yg), _p(pred_dev), K_B, K_N, K_MEL, *tables, 3, step, use_cfg, _a(slot), _s()), "f5k_euler_cfg_items")
    want = IO.euler_items(y, pred, t, K_CFG, K_STEPS, step, use_cfg)
    assert yg.guards_intact() and slot.guards_intact()
    assert yg.value.cpu().numpy().tobytes() == want.tobytes() and slot.value.cpu().numpy().tobytes() == want.tobytes()
    dead = [b for b in range(K_B) if step >= K_STEPS[b]]
    assert all(np.array_equal(want[b], y[b]) for b in dead) and (step == 0 or dead)
    # ... without a slot
    yg = Guarded.like(dev(y))
    _lib.check(lib.f5k_euler_cfg_items(_a(yg), _p(pred_dev), K_B, K_N, K_MEL, *tables, 3, step, use_cfg, None, _s()), "f5k_euler_cfg_items")
    assert yg.guards_intact() and yg.value.cpu().numpy().tobytes() == want.tobytes()
    # the midpoint half step
    mid = Guarded((K_B, K_N, K_MEL), torch.float32)
    _lib.check(lib.f5k_midpoint_half_cfg_items(_p(y_dev), _p(pred_dev), K_B, K_N, K_MEL, *tables, 3, step, use_cfg, _a(mid), _s()),
               "f5k_midpoint_half_cfg_items")
    assert mid.guards_intact()
    assert mid.value.cpu().numpy().tobytes() == IO.midpoint_half_items(y, pred, t, K_CFG, K_STEPS, step, use_cfg).tobytes()


def test_item_update_kernels_refuse_bad_arguments():
    lib = _lib.load()
    y, pred, t = kernel_case()
    held = (dev(y), dev(pred), dev(t), dev(K_CFG, torch.float32), dev(K_STEPS, torch.int32))
    args = (_p(held[0]), _p(held[1]), K_B, K_N, K_MEL, _p(held[2]), _p(held[3]), _p(held[4]))
    assert lib.f5k_euler_cfg_items(*args, 3, 3, 1, None, _s()) == -1                # step == steps_max would read past every grid
    assert lib.f5k_midpoint_half_cfg_items(*args, 3, 0, 1, None, _s()) == -1        # no y_mid
    assert lib.f5k_mod_gather(args[0], args[7], args[0], 2, 3, 6, _s()) == -1       # width % 4


@pytest.mark.parametrize("width", [100, (6 * 2 + 2) * 256])
def test_mod_gather_is_bit_exact(width):
    lib = _lib.load()
    rng = np.random.default_rng(width)
    src = rng.standard_normal((7, width)).astype(np.float32)
    idx = [5, 0, 5, 6, 2]                                              # repeated and out of order
    for rows in (5, 10):                                               # one half, and the conditional half followed by the unconditional
        dst, src_dev, idx_dev = Guarded((rows, width), torch.float32), dev(src), dev(idx, torch.int32)
        _lib.check(lib.f5k_mod_gather(_p(src_dev), _p(idx_dev), _a(dst), rows, len(idx), width, _s()), "f5k_mod_gather")
        assert dst.guards_intact() and dst.value.cpu().numpy().tobytes() == IO.mod_gather(src, idx, rows).tobytes()


# ------------------------------------------------------------------------------------------------ 7. UNetT
def test_unett_mixed_batch_against_the_oracle():
    durs, refs, nts, settings = DURS[:2], REFS[:2], NTS[:2], SETTINGS[:2]
    cond, text, dur, lens = inputs(durs, refs, nts)
    model = build("sample_unett_b2", "f16x3")
    out, traj = (t.cpu() for t in model.sample_items(cond, text, dur, lens=lens, **columns(settings)))
    assert traj.shape == (5, 2, 129, 100)
    for i, (want_out, want_traj) in enumerate(oracle_rows("sample_unett_b2", durs, refs, nts, settings)):
        s = settings[i][0]
        e_traj, e_out = (traj[:s + 1, i] - want_traj).abs().max().item(), (out[i] - want_out).abs().max().item()
        print(f"[items unett f16x3] item {i} {settings[i]}: traj Linf {e_traj:.3e} out Linf {e_out:.3e}")
        assert e_traj < 1e-3 and e_out < 1e-3, f"item {i}"
        assert all(torch.equal(traj[later, i], traj[s, i]) for later in range(s + 1, 5))


# ------------------------------------------------------------------------------------------------ refusals that need an engine
def test_engine_refusals():
    model = build("sample_b1_nfe16", "f32")
    eng = model.transformer.engine()
    cond, text, dur, lens = inputs([20, 12], [6, 4], [5, 3])
    y0 = torch.zeros(2, 20, 100)
    mask = torch.zeros(2, 20, dtype=torch.bool)
    grids = [[0.0, 0.5, 1.0], [0.0, 1.0]]
    with pytest.raises(_lib.F5Error, match="lens required"):
        eng.sample_items(cond, mask, y0, text, grids, [2.0, 2.0], lens=None)
    with pytest.raises(_lib.F5Error, match=r"lens\[1\]=21"):
        eng.sample_items(cond, mask, y0, text, grids, [2.0, 2.0], lens=[20, 21])
    with pytest.raises(_lib.F5Error, match="item 1"):
        eng.sample_items(cond, mask, y0, text, grids, [2.0, float("nan")], lens=[20, 12])
    with pytest.raises(ValueError):
        eng.sample_items(cond, mask, y0, text, grids, [2.0], lens=[20, 12])
    out, traj = eng.sample_items(cond, mask, y0, text, grids, [2.0, 0.0], lens=[20, 12])
    assert traj.shape == (3, 2, 20, 100) and torch.isfinite(traj).all()


# ------------------------------------------------------------------------------------------------ 8. the pool
def test_pool_clients_with_their_own_settings_replayed_from_the_log():
    from test_long_form_gpu import tiny_model, tiny_vocoder
    from test_stream_deliver_gpu import KW, SPEED
    from test_stream_pool_gpu import CLIENTS, TEXTS, bank_of
    import emit_oracle as E

    model, voc = tiny_model(False), tiny_vocoder()
    bank = bank_of(model, False)
    own = {"main": {}, "b": dict(nfe_step=3, cfg_strength=0.5), "c": dict(nfe_step=1, cfg_strength=3.0, seed=11)}
    pool = I.open_pool(model, voc, bank, batch_frames=1500, **KW)
    clients = {name: pool.connect(name, speed=SPEED, **CLIENTS[name], **own[name]) for name in CLIENTS}
    assert clients["main"].sample_kw == pool.sample_kw and clients["b"].sample_kw["steps"] == 3 and clients["c"].sample_kw["seed"] == 11
    reqs, packets = {"main": clients["main"].submit(TEXTS["main"])}, {}
    first = True
    while not pool.idle():
        for r, pk in pool.step():
            packets.setdefault(r.id, []).extend(pk)
        if first:
            reqs["b"], reqs["c"] = clients["b"].submit(TEXTS["b"]), clients["c"].submit(TEXTS["c"])
            first = False
    by_id = {r.id: r for r in reqs.values()}
    assert all(r.done for r in reqs.values())
    stats = pool.stats()
    assert stats["sample_calls"] == stats["ticks"] == len(pool.log)
    mixed = [tick for tick in pool.log if len({tuple(by_id[rid].client.sample_kw.items()) for rid, _ in tick}) > 1]
    assert mixed, "no tick mixes settings: the case lost its point"
    pieces = {rid: [] for rid in by_id}
    with torch.inference_mode():
        for tick in pool.log:
            items = [(by_id[rid], k) for rid, k in tick]
            glens = [bank.frames[r.voice] for r, _ in items]
            rows = torch.tensor([r.voice for r, _ in items], device=DEV)
            kw = {name: [r.client.sample_kw[name] for r, _ in items] for name in ("steps", "cfg_strength", "sway_sampling_coef", "seed")}
            generated, _ = model.sample_items(cond=bank.mel[:, :max(glens)].index_select(0, rows), text=[r.plan["texts"][k] for r, k in items],
                                              duration=torch.tensor([r.plan["durations"][k] for r, k in items]), lens=torch.tensor(glens), **kw)
            wave, wave_lens = voc.decode_ragged(generated.to(torch.float32).permute(0, 2, 1), ends=[r.plan["ends"][k] for r, k in items],
                                                starts=[bank.samples[r.voice] // 256 for r, _ in items])
            wave = I.rescale_to_prompt(wave, bank.rms.index_select(0, rows)[:, None], bank.target_rms)
            for b, (r, _) in enumerate(items):
                pieces[r.id].append(wave[b, :wave_lens[b]])
        for name, r in reqs.items():
            c = r.client
            joined = I.wave_join(pieces[r.id], [0] + [c.fade] * (len(pieces[r.id]) - 1))
            want = I.wave_deliver(model.mel_spec, [joined], out_rate=c.out_rate, sample_format=c.sample_format, final=True)[0].cpu().numpy()
            got = np.concatenate(packets[r.id])
            assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(E.as_bytes(got), E.as_bytes(want)), name
