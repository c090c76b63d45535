"""CPU: the yardstick of the pYIN tests (pyin_oracle.py) pinned where its answer is known -- the octave fixture that raw YIN gets wrong
and the decode gets right, wrong variants that must move an answer -- so that the GPU tests, which hold f5_pitch_candidates and
f5_pitch_decode to it bit for bit, cannot inherit a wrong yardstick; the host tables of metrics.pyin_tables; every refusal of the two
entry points, which comes before anything touches a device; the ABI of the three new symbols."""
import ctypes as C
import math

import numpy as np
import pytest

import pitch_oracle as Y
import pyin_oracle as Q
import f5_tts_amd as P
from f5_tts_amd import _lib
from f5_tts_amd import metrics as M


@pytest.fixture(scope="module")
def tab():
    return M.pyin_tables(Q.SR, Q.FMIN, Q.FMAX)


def test_tables_are_normalised_and_equal_the_oracles(tab):
    assert (tab.tau_min, tab.tau_max) == (Q.TAU_MIN, Q.TAU_MAX) == M.pitch_lags(Q.SR, Q.FMIN, Q.FMAX)
    assert tab.n == 100 and tab.reach == 25 and tab.bins == 185 and tuple(tab.trans.shape) == (185, 51)
    assert abs(math.fsum(tab.w.tolist()) - 1.0) <= 1e-15 and min(tab.w.tolist()) >= 0.0
    for i, row in enumerate(tab.trans.tolist()):
        assert abs(math.fsum(row) - 1.0) <= 1e-15, i
        assert all((v > 0) == (0 <= i + k - tab.reach < tab.bins) for k, v in enumerate(row)), i
    edge = tab.edge.tolist()
    assert all(a < b for a, b in zip(edge, edge[1:])) and all(a < c < b for a, c, b in zip(edge, tab.centre.tolist(), edge[1:]))
    want = Q.tables()
    for name in ("w", "edge", "centre", "trans"):
        assert np.array_equal(getattr(tab, name).numpy(), want[name]), name
    default = M.pyin_tables()
    assert (default.tau_min, default.tau_max, default.bins, default.sample_rate) == (40, 400, 202, 24000)
    with pytest.raises(ValueError, match="bins_per_semitone"):
        M.pyin_tables(bins_per_semitone=16)
    with pytest.raises(ValueError, match="n_thresholds"):
        M.pyin_tables(n_thresholds=257)


def test_a_general_beta_prior_agrees_with_the_closed_form(tab):
    import scipy.special  # noqa: F401  (the optional dependency of a non-default beta: the test environment has it, so no skip)
    general = M.pyin_tables(Q.SR, Q.FMIN, Q.FMAX, beta=(2.0, 18.0000001))
    assert np.abs(general.w.numpy() - tab.w.numpy()).max() < 1e-7 and abs(math.fsum(general.w.tolist()) - 1.0) <= 1e-12


def test_every_candidate_of_every_fixture_lands_in_a_bin(tab):
    edge = tab.edge.numpy()
    seen = 0
    for name in Q.waves():
        _, (count, lag, f0, prob), _ = Q.reference(name)
        for t, c in enumerate(count):
            assert ((edge[0] <= f0[t, :c]) & (f0[t, :c] < edge[-1])).all(), (name, t)
            assert (np.diff(lag[t, :c]) > 0).all() and (prob[t, :c] > 0).all() and not f0[t, c:].any() and not prob[t, c:].any()
            seen += int(c)
    assert seen > 300


def test_the_octave_fixture_fools_yin_and_not_the_decode():
    x = Q.waves()["octave"]
    frames, _, (f0, vp) = Q.reference("octave")
    inn = Q.inner(frames, len(x))
    yin, _ = Y.track(x, hop=Q.HOP, window=Q.WINDOW, tau_min=Q.TAU_MIN, tau_max=Q.TAU_MAX)
    print(f"{inn.sum()} inner frames: YIN bad on {Q.bad_frames(yin, inn)}, the decode on {Q.bad_frames(f0, inn)}; decoded range "
          f"{f0[inn].min():.1f} .. {f0[inn].max():.1f} Hz")
    assert frames == 43 and inn.sum() == 41
    assert Q.bad_frames(yin, inn) >= 3 and (np.abs(yin[inn] - 220.0) < 5.0).sum() >= 3      # the octave below
    assert Q.bad_frames(f0, inn) == 0


def test_noise_is_unvoiced_and_an_onset_is_found():
    frames, (count, _, _, _), (f0, vp) = Q.reference("noise")
    assert not f0.any() and vp.max() < 0.05 and count.max() >= 1
    frames, _, (f0, vp) = Q.reference("onset")
    assert not f0[:15].any() and np.abs(f0[28:45] / 300.0 - 1).max() < 0.01
    frames, (count, _, _, _), (f0, vp) = Q.reference("silence", 0, 0.0)            # no vote without a dip: no candidates, unvoiced
    assert not count.any() and not f0.any() and not vp.any()


@pytest.mark.parametrize("variant", Q.VARIANTS)
def test_every_wrong_variant_moves_an_answer(variant):
    tab, moved = Q.tables(), []
    for name, (t, (count, f0, prob), p_switch) in Q.decode_cases().items():
        if name == "many_bins":                                   # (a second of Python loops, and no other rule than the small cases)
            continue
        kw = dict(edge=t["edge"], centre=t["centre"], reach=t["reach"], trans=t["trans"], p_switch=p_switch)
        a, b = Q.decode(count, f0, prob, **kw), Q.decode(count, f0, prob, variant=variant, **kw)
        if not (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])):
            moved.append(name)
    for name in () if moved else ("octave", "noise"):
        _, _, want = Q.reference(name)
        got = Q.track(Q.waves()[name], tab, variant=variant)
        if not (np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1])):
            moved.append(name)
    print(f"{variant}: differs from the contract on {moved}")
    assert moved


def test_new_symbols_are_bound_and_declared():
    lib = _lib.load()
    for name in ("f5_pitch_candidates", "f5_pitch_decode_bytes", "f5_pitch_decode"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)


def test_pyin_bytes_is_the_librarys_formula():
    lib = _lib.load()
    for frames, bins in ((1, 2), (43, 185), (1 << 22, 512), (0, 185)):
        assert M.pyin_bytes(frames, bins) == lib.f5_pitch_decode_bytes(frames, bins) == 2 * bins * frames


def f64(values):
    return (C.c_double * len(values))(*values)


def test_candidates_refusals_need_no_gpu():
    """Every refusal comes before anything touches the device: safe to call here with pointers that are never dereferenced."""
    lib = _lib.load()
    one = C.c_void_p(64)
    w = [0.25] * 4

    def call(P_=1, start=(0,), lens=(1000,), rate=24000, hop=256, centre=0, frames=(4,), W=256, lo=20, hi=160, N=4, w=w, absent=0.01,
             base=one, count=one, lag=one, f0=one, prob=one):
        return lib.f5_pitch_candidates(base, P_, (C.c_int64 * len(start))(*start), _lib.int_array(list(lens)), rate, hop, centre,
                                       _lib.int_array(list(frames)), W, lo, hi, N, f64(w) if w is not None else None, absent, count, lag,
                                       f0, prob, None)
    nan, inf = float("nan"), float("inf")
    for kw, needle in ((dict(P_=0), "P"), (dict(P_=65536), "P"), (dict(W=63), "window"), (dict(W=2049), "window"), (dict(lo=1), "tau_min"),
                       (dict(lo=160), "tau_min"), (dict(hi=1025), "tau_max"), (dict(lens=(0,)), "item 0 has len"),
                       (dict(start=(-1,)), "item 0 has start"), (dict(frames=(0,)), "item 0 has frames"), (dict(rate=0), "sample_rate"),
                       (dict(hop=0), "hop"), (dict(centre=-1), "first_centre"), (dict(P_=2, start=(0, 0), lens=(9, 9), frames=(1 << 22, 1)),
                                                                                  "more than 4194304 frames"),
                       (dict(N=0), "N = 0"), (dict(N=257, w=[0.0] * 257), "N = 257"), (dict(w=None), "null w_host"),
                       (dict(w=[0.5, nan, 0.25, 0.25]), "w_host[1] is not finite"), (dict(w=[0.5, 0.25, inf, 0.25]), "w_host[2] is not finite"),
                       (dict(w=[0.5, 0.5, 0.5, -0.5]), "w_host[3] = -0.5 is negative"), (dict(absent=-0.01), "p_absent"),
                       (dict(absent=1.01), "p_absent"), (dict(absent=nan), "p_absent"), (dict(base=None), "null base"),
                       (dict(count=None), "null cand_count"), (dict(lag=None), "null cand_lag"), (dict(f0=None), "null cand_f0"),
                       (dict(prob=None), "null cand_prob")):
        rc = call(**kw)
        msg = lib.f5_last_error().decode()
        assert rc == -1 and "f5_pitch_candidates" in msg and needle in msg, (kw, msg)


def test_decode_refusals_need_no_gpu():
    lib = _lib.load()
    one = C.c_void_p(64)
    t = Q.small_tables(4, 1)
    edge, centre, trans = t["edge"].tolist(), t["centre"].tolist(), t["trans"].reshape(-1).tolist()

    def call(N=3, P_=1, frames=(5,), M_=4, edge=edge, centre=centre, reach=1, trans=trans, p_switch=0.01, work=one, work_bytes=40,
             count=one, cf0=one, prob=one, f0=one, vp=one):
        arr = lambda v: f64(v) if v is not None else None          # noqa: E731
        return lib.f5_pitch_decode(count, cf0, prob, N, P_, _lib.int_array(list(frames)) if frames is not None else None, M_, arr(edge),
                                   arr(centre), reach, arr(trans), p_switch, work, work_bytes, f0, vp, None)
    nan = float("nan")
    bad_edge = list(edge)
    bad_edge[2] = bad_edge[1]
    for kw, needle in ((dict(N=0), "N = 0"), (dict(N=257), "N = 257"), (dict(P_=0), "P"), (dict(P_=65536), "P"), (dict(M_=1), "M = 1"),
                       (dict(M_=513), "M = 513"), (dict(reach=0), "reach = 0"), (dict(reach=64), "reach = 64"), (dict(p_switch=0.0), "p_switch"),
                       (dict(p_switch=1.0), "p_switch"), (dict(p_switch=nan), "p_switch"), (dict(edge=None), "null edge_host"),
                       (dict(centre=None), "null centre_host"), (dict(trans=None), "null trans_host"),
                       (dict(edge=edge[:3] + [nan, edge[4]]), "edge_host[3] is not finite"), (dict(edge=bad_edge), "not strictly ascending at 1"),
                       (dict(edge=edge[::-1]), "not strictly ascending at 0"), (dict(centre=centre[:2] + [float("inf")] + centre[3:]),
                                                                                 "centre_host[2] is not finite"),
                       (dict(trans=trans[:5] + [nan] + trans[6:]), "trans_host[5] is not finite"),
                       (dict(trans=trans[:7] + [-0.5] + trans[8:]), "trans_host[7] = -0.5 is negative"), (dict(frames=(0,)), "item 0 has frames"),
                       (dict(frames=None), "null frames_host"), (dict(P_=2, frames=(1 << 22, 1)), "more than 4194304 frames"),
                       (dict(work_bytes=39), "workspace_bytes = 39 (need 40"), (dict(work=None), "null workspace"),
                       (dict(count=None), "null cand_count"), (dict(cf0=None), "null cand_f0"), (dict(prob=None), "null cand_prob"),
                       (dict(f0=None), "null f0"), (dict(vp=None), "null voiced_prob")):
        rc = call(**kw)
        msg = lib.f5_last_error().decode()
        assert rc == -1 and "f5_pitch_decode" in msg and needle in msg, (kw, msg)


def test_given_tables_must_match_the_call(tab):
    """Tables bring their own lag range; a sample rate or an fmin / fmax that says otherwise is refused, not ignored (before any device)."""
    import torch
    wave = [torch.zeros(2000)]
    for fn in (M.pitch_candidates, M.pitch_track_pyin):
        with pytest.raises(ValueError, match="built for 24000 Hz"):
            fn(wave, sample_rate=16000, tables=tab)
        with pytest.raises(ValueError, match=r"built for the lags 20 \.\. 160"):
            fn(wave, fmin=60.0, fmax=600.0, tables=tab)
        with pytest.raises(ValueError, match="both fmin and fmax"):
            fn(wave, fmin=60.0, tables=tab)
        with pytest.raises(ValueError, match="weights"):
            fn(wave, tables=M.PyinTables(24000, 20, 160, torch.zeros(2, 2), tab.edge, tab.centre, tab.reach, tab.trans))
    assert M._tables_for("x", tab, Q.SR, Q.FMIN, Q.FMAX) is tab and M._tables_for("x", tab, Q.SR, None, None) is tab
    assert M._tables_for("x", None, Q.SR, None, None).tau_max == 400


def test_heldout_prosody_refuses_an_unknown_tracker():
    with pytest.raises(ValueError, match="pitch = 'nonsense'"):
        P.infer.heldout_prosody(None, None, [], pitch="nonsense")
