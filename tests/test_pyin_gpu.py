"""GPU: f5_pitch_candidates and f5_pitch_decode (csrc/pitch.hip) against the float64 restatement of their contract in pyin_oracle.py,
bit for bit -- every operation of the contract is a correctly rounded f64 add, multiply, divide or compare in a fixed order, and the
one order-free step, the frame's maximum, is exact -- then metrics.pitch_track_pyin on the fixture that raw YIN gets wrong, ragged
batches, NaN containment, guard words, refusals, and infer.heldout_prosody(pitch="pyin") on a tiny synthetic DiT.  test_pyin.py pins
the oracle itself."""
import ctypes as C

import numpy as np
import pytest
import torch

import dtw_oracle as O
import pitch_oracle as Y
import prosody_oracle as R
import pyin_oracle as Q
import test_prosody_gpu as G
import f5_tts_amd as P
from f5_tts_amd import _lib
from f5_tts_amd import metrics as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRID = dict(sample_rate=Q.SR, hop=Q.HOP, window=Q.WINDOW)
S64, S32, S8 = 0x7FF8A5A5A5A5A5A5, 0x5A5A5A5A, 0x5A


@pytest.fixture(scope="module")
def tab():
    return M.pyin_tables(Q.SR, Q.FMIN, Q.FMAX)


def bits(t):
    return t.cpu().contiguous().view(torch.int64)


def same_f64(got, want):
    """A device f64 tensor against a NumPy f64 array of the same shape, bit for bit."""
    return torch.equal(bits(got), torch.from_numpy(np.ascontiguousarray(want, dtype=np.float64)).view(torch.int64))


def device_tables(t, n=1):
    """One of the oracle's hand-made table sets as the package takes them."""
    return M.PyinTables(Q.SR, Q.TAU_MIN, Q.TAU_MAX, torch.full((n,), 1.0 / n, dtype=torch.float64), torch.from_numpy(t["edge"]),
                        torch.from_numpy(t["centre"]), int(t["reach"]), torch.from_numpy(t["trans"]))


def frames_of(x, first_centre):
    return len(x) // Q.HOP + (1 if first_centre == 0 else 0)


# ---------------------------------------------------------------------------------------------------- stage 1
@pytest.mark.parametrize("first_centre", [0, Q.HOP // 2])
def test_candidates_equal_the_oracle_on_every_fixture(tab, first_centre):
    waves = Q.waves()
    frames = [frames_of(x, first_centre) for x in waves.values()]
    count, lag, f0, prob, got = M.pitch_candidates([torch.from_numpy(x).to(DEV) for x in waves.values()], frames=frames,
                                                   first_centre=first_centre, tables=tab, **GRID)
    assert got == frames and count.shape == (sum(frames),) and lag.shape == f0.shape == prob.shape == (sum(frames), 100)
    at = 0
    for (name, x), n in zip(waves.items(), frames):
        want_frames, (wc, wl, wf, wp), _ = Q.reference(name, first_centre)
        assert want_frames == n
        sl = slice(at, at + n)
        at += n
        print(f"{name} (first_centre {first_centre}): {n} frames, {int(wc.sum())} candidates, at most {int(wc.max())} in a frame")
        assert torch.equal(count[sl].cpu(), torch.from_numpy(wc)) and torch.equal(lag[sl].cpu(), torch.from_numpy(wl)), name
        assert same_f64(f0[sl], wf) and same_f64(prob[sl], wp), name


@pytest.mark.parametrize("window, fmin, fmax, bps", [(64, 1500.0, 12000.0, 5), (2048, 24000 / 1024, 12000.0, 4)])
def test_candidates_at_the_smallest_and_the_largest_window_and_lag_range(window, fmin, fmax, bps):
    t = M.pyin_tables(Q.SR, fmin, fmax, n_thresholds=8, bins_per_semitone=bps)
    assert (t.tau_min, t.tau_max) == ((2, 16) if window == 64 else (2, 1024))
    waves = dict(tone=Y.harmonic(440, 0.12, seed=1), high=Y.harmonic(3000, 0.1, seed=2, harmonics=2), noise=Y.noise(0.1, seed=3),
                 one=Y.harmonic(440, 0.12, seed=1)[:1], zeros=np.zeros(700, np.float32), square=Y.square(150.0, 0.12))
    got = M.pitch_candidates([torch.from_numpy(x).to(DEV) for x in waves.values()], sample_rate=Q.SR, hop=Q.HOP, window=window, tables=t)
    at = 0
    for (name, x), n in zip(waves.items(), got[4]):
        wc, wl, wf, wp = Q.candidates(x, w=t.w.numpy(), window=window, tau_min=t.tau_min, tau_max=t.tau_max)
        sl = slice(at, at + n)
        at += n
        print(f"window {window} {name}: {n} frames, {int(wc.sum())} candidates")
        assert torch.equal(got[0][sl].cpu(), torch.from_numpy(wc)) and torch.equal(got[1][sl].cpu(), torch.from_numpy(wl)), name
        assert same_f64(got[2][sl], wf) and same_f64(got[3][sl], wp), name


# ---------------------------------------------------------------------------------------------------- stage 2
def device_decode(t, table, p_switch, frames=None):
    count, f0, prob = table
    return M.pitch_decode(torch.from_numpy(count).to(DEV), torch.from_numpy(f0).to(DEV), torch.from_numpy(prob).to(DEV),
                          frames or [len(count)], device_tables(t), p_switch=p_switch)


CASES = ["hand_made", "all_equal", "full_reach_and_flip", "two_bins", "many_bins", "reach_over_bins", "one_frame", "no_candidates",
         "tot_over_one", "unreachable_jump", "edge_rows", "near_ties", "voicing_ties", "equal_probs_in_a_bin", "on_an_edge"]


@pytest.mark.parametrize("case", CASES)
def test_decode_equals_the_oracle(case):
    t, table, p_switch = Q.decode_cases()[case]
    want_f0, want_vp = Q.decode(*table, edge=t["edge"], centre=t["centre"], reach=t["reach"], trans=t["trans"], p_switch=p_switch)
    f0, vp = device_decode(t, table, p_switch)
    print(f"{case}: M {t['M']}, reach {t['reach']}, {len(want_f0)} frames, {(want_f0 > 0).sum()} voiced, voiced_prob at most {want_vp.max()!r}")
    assert same_f64(f0, want_f0) and same_f64(vp, want_vp)
    if case == "tot_over_one":
        assert want_vp.max() > 1.0
    assert sorted(Q.decode_cases()) == sorted(CASES)              # (no case of the oracle left out)
    if case == "voicing_ties":                                    # the same voicing on ties, unvoiced at the end
        assert not want_f0.any()
    if case == "full_reach_and_flip":                            # +reach, +reach, off, on again, -reach, -reach
        assert [int(round(12 * np.log2(v / 100.0) - 0.5)) if v else -1 for v in want_f0] == [2, 4, 6, -1, 4, 2, 0]


def test_decode_takes_the_cases_of_one_table_set_as_one_ragged_batch():
    cases = Q.decode_cases()
    names = ["hand_made", "one_frame", "no_candidates", "unreachable_jump", "edge_rows"]    # all on small_tables(12, 3)
    t, N = cases[names[0]][0], 4
    count = np.concatenate([cases[k][1][0] for k in names])
    f0 = np.concatenate([np.pad(cases[k][1][1], ((0, 0), (0, N - cases[k][1][1].shape[1]))) for k in names])
    prob = np.concatenate([np.pad(cases[k][1][2], ((0, 0), (0, N - cases[k][1][2].shape[1]))) for k in names])
    frames = [len(cases[k][1][0]) for k in names]
    got_f0, got_vp = device_decode(t, (count, f0, prob), 0.01, frames)
    want = [Q.decode(*cases[k][1], edge=t["edge"], centre=t["centre"], reach=t["reach"], trans=t["trans"], p_switch=0.01) for k in names]
    assert same_f64(got_f0, np.concatenate([w[0] for w in want])) and same_f64(got_vp, np.concatenate([w[1] for w in want]))


# ---------------------------------------------------------------------------------------------------- both stages
def test_the_octave_fixture_is_decoded_right_where_yin_on_the_same_buffer_is_not(tab):
    x = Q.waves()["octave"]
    wave = torch.from_numpy(x).to(DEV)
    frames, _, (want_f0, want_vp) = Q.reference("octave")
    f0, vp, got = M.pitch_track_pyin([wave], tables=tab, **GRID)
    yin, _, _ = M.pitch_track([wave], fmin=Q.FMIN, fmax=Q.FMAX, **GRID)
    inn = Q.inner(frames, len(x))
    bad_yin, bad_pyin = Q.bad_frames(yin.cpu().numpy(), inn), Q.bad_frames(f0.cpu().numpy(), inn)
    print(f"{inn.sum()} inner frames: pitch_track bad on {bad_yin}, pitch_track_pyin on {bad_pyin}")
    assert got == [frames] and same_f64(f0, want_f0) and same_f64(vp, want_vp)
    assert bad_pyin == 0 and bad_yin == 4 == Q.bad_frames(Y.track(x, hop=Q.HOP, window=Q.WINDOW, tau_min=Q.TAU_MIN, tau_max=Q.TAU_MAX)[0], inn)


def test_tracks_equal_the_oracle_on_every_fixture(tab):
    waves = Q.waves()
    f0, vp, frames = M.pitch_track_pyin([torch.from_numpy(x).to(DEV) for x in waves.values()], tables=tab, **GRID)
    at = 0
    for name, n in zip(waves, frames):
        _, _, (want_f0, want_vp) = Q.reference(name)
        print(f"{name}: {n} frames, {(want_f0 > 0).sum()} voiced")
        assert same_f64(f0[at:at + n], want_f0) and same_f64(vp[at:at + n], want_vp), name
        at += n


def test_ragged_batch_of_five_equals_each_item_alone_in_any_order(tab):
    w = Q.waves()
    five = [torch.from_numpy(x).to(DEV) for x in (w["octave"], w["glide"][:Q.HOP + 1], w["noise"], w["onset"], w["square"][:5000])]
    f0, vp, frames = M.pitch_track_pyin(five, tables=tab, **GRID)
    assert frames == [x.numel() // Q.HOP + 1 for x in five]
    pieces = list(zip(bits(f0).split(frames), bits(vp).split(frames)))
    for x, (p0, pv) in zip(five, pieces):
        a0, av, _ = M.pitch_track_pyin([x], tables=tab, **GRID)
        assert torch.equal(bits(a0), p0) and torch.equal(bits(av), pv)
    perm = [3, 0, 4, 2, 1]
    g0, gv, gf = M.pitch_track_pyin([five[i] for i in perm], tables=tab, **GRID)
    again = list(zip(bits(g0).split(gf), bits(gv).split(gf)))
    for k, i in enumerate(perm):
        assert torch.equal(again[k][0], pieces[i][0]) and torch.equal(again[k][1], pieces[i][1])
    # rows of a [B, L_max] tensor with lens, as decode_ragged returns them: read in place; default tables = the ones of the range
    L = max(x.numel() for x in five)
    wav = torch.full((5, L), float("nan"), device=DEV)
    for k, x in enumerate(five):
        wav[k, :x.numel()] = x
    r0, rv, rf = M.pitch_track_pyin(wav, [x.numel() for x in five], fmin=Q.FMIN, fmax=Q.FMAX, **GRID)
    assert rf == frames and torch.equal(bits(r0), bits(f0)) and torch.equal(bits(rv), bits(vp))


def guarded(n, dtype, word):
    return torch.full((8 + n + 8,), word, dtype=dtype, device=DEV)


def intact(t, word, payload=None):
    h = t.cpu().tolist()
    return h[:8] == [word] * 8 and h[-8:] == [word] * 8 and (payload is None or h[8:-8] == payload)


def test_a_nan_sample_stays_inside_its_item_and_guard_words_stay_intact(tab):
    w = Q.waves()
    three = [torch.from_numpy(w[k]).to(DEV) for k in ("glide", "octave", "onset")]
    f0, vp, frames = M.pitch_track_pyin(three, tables=tab, **GRID)
    bad = [t.clone() for t in three]
    bad[1][5000] = float("nan")
    g0, gv, _ = M.pitch_track_pyin(bad, tables=tab, **GRID)
    keep = torch.ones(sum(frames), dtype=torch.bool)
    keep[frames[0]:frames[0] + frames[1]] = False
    assert torch.equal(bits(g0)[keep], bits(f0)[keep]) and torch.equal(bits(gv)[keep], bits(vp)[keep])
    mid = slice(frames[0], frames[0] + frames[1])
    assert not torch.equal(bits(gv)[mid], bits(vp)[mid]) and torch.isfinite(g0).all() and torch.isfinite(gv).all()
    # the raw calls between guard words, the workspace too
    total, N, bins = sum(frames), tab.n, tab.bins
    cand = M.pitch_candidates(three, tables=tab, **GRID)
    lib, stream = _lib.load(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    base = min(t.data_ptr() for t in three)
    gc, gl = guarded(total, torch.int32, S32), guarded(total * N, torch.int32, S32)
    gf, gp = guarded(total * N, torch.int64, S64), guarded(total * N, torch.int64, S64)
    go, gv2, gw = guarded(total, torch.int64, S64), guarded(total, torch.int64, S64), guarded(M.pyin_bytes(total, bins), torch.uint8, S8)
    ptr = lambda t: C.c_void_p(t.data_ptr() + 8 * t.element_size())          # noqa: E731
    f64p = lambda t: C.cast(C.c_void_p(t.data_ptr()), C.POINTER(C.c_double))  # noqa: E731

    def raw_candidates(n=N, window=Q.WINDOW):
        return lib.f5_pitch_candidates(C.c_void_p(base), 3, (C.c_int64 * 3)(*[(t.data_ptr() - base) // 4 for t in three]),
                                       _lib.int_array([t.numel() for t in three]), Q.SR, Q.HOP, 0, _lib.int_array(frames), window, tab.tau_min,
                                       tab.tau_max, n, f64p(tab.w), 0.01, ptr(gc), ptr(gl), ptr(gf), ptr(gp), stream)

    def raw_decode(work_bytes=M.pyin_bytes(total, bins), p_switch=0.01):
        return lib.f5_pitch_decode(ptr(gc), ptr(gf), ptr(gp), N, 3, _lib.int_array(frames), bins, f64p(tab.edge), f64p(tab.centre), tab.reach,
                                   f64p(tab.trans), p_switch, ptr(gw), work_bytes, ptr(go), ptr(gv2), stream)
    with torch.cuda.device(DEV):
        assert raw_candidates() == 0 and raw_decode() == 0
        torch.cuda.synchronize()
        assert intact(gc, S32, cand[0].cpu().tolist()) and intact(gl, S32, cand[1].cpu().reshape(-1).tolist())
        assert intact(gf, S64, bits(cand[2]).reshape(-1).tolist()) and intact(gp, S64, bits(cand[3]).reshape(-1).tolist())
        assert intact(go, S64, bits(f0).tolist()) and intact(gv2, S64, bits(vp).tolist()) and intact(gw, S8)
        # refused calls write nothing: fill everything the calls write, refuse, look
        for t, word in ((go, S64), (gv2, S64), (gw, S8)):
            t.fill_(word)
        err = lambda: lib.f5_last_error().decode()                            # noqa: E731
        assert raw_decode(work_bytes=M.pyin_bytes(total, bins) - 1) == -1 and "workspace_bytes" in err()
        assert raw_decode(p_switch=1.0) == -1 and "p_switch" in err()
        for t, word in ((gc, S32), (gl, S32), (gf, S64), (gp, S64)):
            t.fill_(word)
        assert raw_candidates(n=257) == -1 and "N = 257" in err()
        assert raw_candidates(window=4096) == -1 and "window" in err()
        torch.cuda.synchronize()
    assert all(t.cpu().tolist() == [word] * t.numel() for t, word in ((gc, S32), (gl, S32), (gf, S64), (gp, S64), (go, S64), (gv2, S64), (gw, S8)))


def test_an_infinite_sample_leaves_its_frames_without_candidates(tab):
    """inf in the window makes d = S = inf and d' = inf / inf = NaN: the contract's "no candidates", not a vote on a NaN."""
    x = Q.waves()["octave"].copy()
    x[5000] = np.inf
    frames = frames_of(x, 0)
    with np.errstate(all="ignore"):
        wc, wl, wf, wp = Q.candidates(x, w=tab.w.numpy(), frames=frames)
        want_f0, want_vp = Q.decode(wc, wf, wp, edge=tab.edge.numpy(), centre=tab.centre.numpy(), reach=tab.reach, trans=tab.trans.numpy())
    count, lag, f0, prob, _ = M.pitch_candidates([torch.from_numpy(x).to(DEV)], tables=tab, **GRID)
    assert (wc == 0).sum() == 2 and (wc > 0).sum() == frames - 2          # L = 417 samples: the two frames that hold sample 5000
    assert torch.equal(count.cpu(), torch.from_numpy(wc)) and torch.equal(lag.cpu(), torch.from_numpy(wl)) and same_f64(f0, wf) and same_f64(prob, wp)
    t0, tv, _ = M.pitch_track_pyin([torch.from_numpy(x).to(DEV)], tables=tab, **GRID)
    assert same_f64(t0, want_f0) and same_f64(tv, want_vp)


# ---------------------------------------------------------------------------------------------------- the driver
PITCH = dict(window=Q.WINDOW, fmin=Q.FMIN, fmax=Q.FMAX)


def heldout_items():
    """test_prosody_gpu's items an octave up, inside the tests' 150 .. 1200 Hz: voiced tones with vibrato, noise inside the second."""
    g = torch.Generator().manual_seed(21)
    items = []
    for k, (p, t) in enumerate(zip(G.PROMPT, G.TARGET)):
        n = (t - 1) * Q.HOP + 17 * (k + 1)
        wave = G.vibrato(n, 280.0 + 80 * k, 0.06, 5.0 + k, seed=60 + k)
        if k == 1:
            wave[3000:6000] = Y.noise(seed=9)[:3000]
        items.append((torch.from_numpy(O.random_walk_mel(40 + k, p)), torch.randint(0, 40, (5 + k,), generator=g), torch.from_numpy(wave),
                      torch.randint(0, 40, (7 + 2 * k,), generator=g)))
    return items


class ToneVocoder:
    """decode_ragged's interface, returning prepared tones of the right lengths near the targets' pitch, silent at their start."""
    def __init__(self):
        self.waves = []

    def decode_ragged(self, mel, ends, starts=None, gain=None):
        lens = [(int(e) - int(s) - 1) * Q.HOP for e, s in zip(ends, starts)]
        host = [G.vibrato(n, 300.0 + 70 * b, 0.05, 4.0 + b, seed=80 + b) for b, n in enumerate(lens)]
        for w in host:
            w[:1500] = 0.0
        wav = torch.zeros(len(lens), max(lens))
        for b, w in enumerate(host):
            wav[b, :len(w)] = torch.from_numpy(w)
        self.waves.append(host)
        return wav.to(mel.device), lens


def test_heldout_prosody_with_pyin_equals_the_oracle_chain_and_yin_stays_the_default(tab):
    model, items, voc = G.tiny(adapters=False), heldout_items(), ToneVocoder()
    tmels = G.target_mels(model, items)
    assert [t.shape[0] for t in tmels] == list(G.TARGET)
    got = P.infer.heldout_prosody(model, voc, items, pitch="pyin", **PITCH, **G.KW)[None]
    plain = P.infer.heldout_prosody(model, voc, items, **PITCH, **G.KW)[None]
    named = P.infer.heldout_prosody(model, voc, items, pitch="yin", **PITCH, **G.KW)[None]
    assert repr(named) == repr(plain) and got["mcd"] == plain["mcd"] and set(got) == set(plain)       # (repr: NaN-proof, bit-exact)
    assert [set(r) for r in got["per_item"]] == [set(r) for r in plain["per_item"]]
    otab = Q.tables()
    grid = dict(hop=Q.HOP, window=Q.WINDOW)
    out, ends = G.sample_alone(model, items, None)
    pooled = dict(cells=0, both_voiced=0, vuv_mismatch=0, **{k: 0.0 for k in R.SUMS})
    for u, it in enumerate(items):
        p = it[0].shape[0]
        t_track = Q.track(it[2].numpy(), otab, frames=G.TARGET[u], **grid)[0]
        g_track = Q.track(voc.waves[0][u], otab, frames=ends[u] - p, **grid)[0]
        _, path = R.alignment(out[u, p:ends[u]].numpy(), tmels[u].numpy())
        want, have = R.fold(g_track, t_track, path), got["per_item"][u]
        for k in ("cells", "both_voiced", "vuv_mismatch"):
            assert have[k] == want[k], (u, k, have[k], want[k])
            pooled[k] += want[k]
        # test_prosody_gpu's bound on the fold: N terms of magnitude below log2(1264)^2 < 107, a few ulp on each logarithm and product,
        # N additions in any order
        N = want["both_voiced"]
        bound = N * 107.0 * (N + 16) * 2.0 ** -53
        for k in R.SUMS:
            assert abs(have[k] - want[k]) <= bound, (u, k, have[k], want[k], bound)
            pooled[k] += want[k]
        print(f"item {u}: {want['cells']} cells, {N} voiced on both sides, {want['vuv_mismatch']} on one")
        assert N > 10
    ref = P.infer.prosody_numbers(pooled)
    for k in ("f0_rmse_cents", "f0_corr", "vuv_error"):
        print(f"{k}: pyin {got[k]!r} (oracle chain {ref[k]!r}), yin {plain[k]!r}")
        assert np.isfinite(got[k]) and abs(got[k] - ref[k]) <= 1e-9 * max(1.0, abs(ref[k]))
    assert pooled["vuv_mismatch"] > 0
