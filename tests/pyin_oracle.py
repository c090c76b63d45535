"""The yardstick of the pYIN tests: the contract of include/f5_hip.h (f5_pitch_candidates, f5_pitch_decode) restated in NumPy float64,
sharing no code with the package (the frame window and d' are pitch_oracle's, the yardstick of f5_pitch_track, as the contract says).

  stage 1   thresholds s_i = i / N, i = 1 .. N ascending; tau_i = YIN's choice at s_i, prob[tau_i] += w_i; none under the threshold:
            prob[tau_g] += w_i * p_absent, tau_g the first arg-min of d' over the range.  Candidates: the lags with prob > 0,
            ascending, with YIN's parabolic f0.  A NaN anywhere in d'(1 .. tau_max + 1): no candidates.
  stage 2   bin of a candidate = #{j in [1, M - 1]: edge[j] <= f0}; ov[m], tot summed in array order; ou = max(0, 1 - tot) / M; both
            floored at 2^-60; delta = 1 before frame 0; inner_v(j) = max_i delta_prev(v, i) * trans[i][j - i + reach] (i ascending,
            smallest i on ties); c = inner_same * (1 - p_switch) unless inner_other * p_switch is larger; delta = obs * c; every delta
            divided by the frame's maximum (if > 0); end state: unvoiced before voiced, smallest bin; output: the f0 of the largest
            candidate of the state's bin (first on ties), centre[m] without one, 0 where unvoiced; voiced_prob = tot.

Every sum and every maximum whose order matters runs in a Python loop.  VARIANTS names decoders and voters a kernel could plausibly be
instead; DECODE_CASES are hand-made candidate tables for the decode alone."""
import functools
import math

import numpy as np

import pitch_oracle as Y

FLOOR = 2.0 ** -60
VARIANTS = ("per_frame_argmax", "ties_largest_bin", "unnormalised_rows", "no_floor", "voicing_then_band", "absent_full_weight",
            "voicing_tie_to_other", "end_voiced_first", "last_equal_candidate", "edge_strict")
# the shapes of the tests: 24 kHz, window 256, lags 20 .. 160 (150 .. 1200 Hz)
SR, HOP, WINDOW, FMIN, FMAX = 24000, 256, 256, 150.0, 1200.0
TAU_MIN, TAU_MAX = 20, 160


# ---------------------------------------------------------------------------------------------------- tables
def beta_weights(n=100):
    """w_i = F(i / n) - F((i - 1) / n), F the Beta(2, 18) CDF in closed form."""
    def cdf(s):
        return 1.0 - (1.0 - s) ** 19 - 19.0 * s * (1.0 - s) ** 18
    return np.array([cdf(i / n) - cdf((i - 1) / n) for i in range(1, n + 1)], dtype=np.float64)


def tables(sample_rate=SR, tau_min=TAU_MIN, tau_max=TAU_MAX, n=100, bins_per_semitone=5, max_semitones=5):
    lo, hi = sample_rate / (tau_max + 1), sample_rate / (tau_min - 1)
    M = int(math.ceil(12 * bins_per_semitone * math.log2(hi / lo)))
    edge = np.array([lo * (hi / lo) ** (m / M) for m in range(M + 1)])
    centre = np.array([lo * (hi / lo) ** ((m + 0.5) / M) for m in range(M)])
    reach = bins_per_semitone * max_semitones
    trans = np.zeros((M, 2 * reach + 1))
    for i in range(M):
        for k in range(2 * reach + 1):
            if 0 <= i + k - reach < M:
                trans[i, k] = reach + 1 - abs(k - reach)
        trans[i] = trans[i] / math.fsum(trans[i])
    return dict(n=n, w=beta_weights(n), tau_min=tau_min, tau_max=tau_max, M=M, edge=edge, centre=centre, reach=reach, trans=trans)


# ---------------------------------------------------------------------------------------------------- stage 1
def candidates(x, *, w, p_absent=0.01, sample_rate=SR, hop=HOP, first_centre=0, frames=None, window=WINDOW, tau_min=TAU_MIN,
               tau_max=TAU_MAX, variant=None):
    """(count int32 [F], lag int32 [F, N], f0 [F, N], prob [F, N]); the slots behind a frame's count are zeros."""
    x = np.asarray(x, dtype=np.float32)
    N = len(w)
    frames = len(x) // hop + 1 if frames is None else frames
    X = Y.frame_matrix(x, frames, hop, first_centre, window + tau_max + 1)
    dn, _ = Y.normalised_difference(X, window, tau_max)
    count = np.zeros(frames, np.int32)
    lag = np.zeros((frames, N), np.int32)
    f0, prob = np.zeros((frames, N)), np.zeros((frames, N))
    for t in range(frames):
        row = dn[t]
        if np.isnan(row[1:tau_max + 2]).any():
            continue
        acc = {}
        tau_g = tau_min
        for k in range(tau_min + 1, tau_max + 1):
            if row[k] < row[tau_g]:
                tau_g = k
        for i in range(1, N + 1):
            s = float(i) / float(N)
            tau = 0
            for k in range(tau_min, tau_max + 1):
                if row[k] < s:
                    tau = k
                    break
            if tau:
                while tau + 1 <= tau_max and row[tau + 1] < row[tau]:
                    tau += 1
                acc[tau] = acc.get(tau, 0.0) + w[i - 1]
            else:
                acc[tau_g] = acc.get(tau_g, 0.0) + (w[i - 1] if variant == "absent_full_weight" else w[i - 1] * p_absent)
        c = 0
        for tau in sorted(acc):
            if not acc[tau] > 0.0:
                continue
            a, b, cc = row[tau - 1], row[tau], row[tau + 1]
            den = a - 2.0 * b + cc
            delta = (0.5 * (a - cc)) / den if den > 0 else 0.0
            delta = -0.5 if delta < -0.5 else (0.5 if delta > 0.5 else delta)
            lag[t, c], f0[t, c], prob[t, c] = tau, float(sample_rate) / (float(tau) + delta), acc[tau]
            c += 1
        count[t] = c
    return count, lag, f0, prob


# ---------------------------------------------------------------------------------------------------- stage 2
def bin_of(edge, f):
    M = len(edge) - 1
    return sum(1 for j in range(1, M) if edge[j] <= f)


def decode(count, f0, prob, *, edge, centre, reach, trans, p_switch=0.01, variant=None, detail=False):
    """(f0 [F], voiced_prob [F]) of ONE item; detail=True adds the last frame's delta [2, M] (0: unvoiced, 1: voiced)."""
    edge, centre, trans = np.asarray(edge, np.float64), np.asarray(centre, np.float64), np.asarray(trans, np.float64)
    M, F, N = len(centre), len(count), f0.shape[1]
    if variant == "unnormalised_rows":               # the triangle as it is, rows not divided by their sums
        trans = np.where(trans > 0, reach + 1.0 - np.abs(np.arange(2 * reach + 1) - reach)[None, :], 0.0)
    inner_edges = edge[1:M]
    stay = 1.0 - p_switch
    delta = np.ones((2, M))
    back = np.zeros((F, 2, M, 2), np.int64)          # (source voicing, source bin)
    out, vp = np.zeros(F), np.zeros(F)
    bins_of = []
    for t in range(F):
        cnt = min(max(int(count[t]), 0), N)
        side = "left" if variant == "edge_strict" else "right"        # (left: edge[j] < f0, a candidate on an edge one bin down)
        bins = [int(np.searchsorted(inner_edges, f0[t, c], side=side)) if not np.isnan(f0[t, c]) else 0 for c in range(cnt)]
        bins_of.append(bins)
        ov, tot = np.zeros(M), 0.0
        for c in range(cnt):
            ov[bins[c]] = ov[bins[c]] + prob[t, c]
            tot = tot + prob[t, c]
        vp[t] = tot
        ou = max(0.0, 1.0 - tot) / float(M)
        if variant == "per_frame_argmax":
            if cnt and tot > 0.5:
                best = 0
                for c in range(1, cnt):
                    if prob[t, c] > prob[t, best]:
                        best = c
                out[t] = f0[t, best]
            continue
        if variant != "no_floor":
            ou = max(ou, FLOOR)
            ov = np.maximum(ov, FLOOR)
        new = np.zeros((2, M))
        for j in range(M):
            inner, arg = [0.0, 0.0], [0, 0]
            for v in (0, 1):
                best, at = -1.0, max(0, j - reach)
                for i in range(max(0, j - reach), min(M - 1, j + reach) + 1):
                    p = delta[v, i] * trans[i, j - i + reach]
                    if p > best or (variant == "ties_largest_bin" and p == best):
                        best, at = p, i
                inner[v], arg[v] = best, at
            for v2 in (0, 1):
                u = 1 - v2
                if variant == "voicing_then_band":
                    # the two multiplications in the other order: (delta * factor) * trans, maximised over i per source voicing
                    cand = []
                    for v, factor in ((v2, stay), (u, p_switch)):
                        best, at = -1.0, max(0, j - reach)
                        for i in range(max(0, j - reach), min(M - 1, j + reach) + 1):
                            p = (delta[v, i] * factor) * trans[i, j - i + reach]
                            if p > best:
                                best, at = p, i
                        cand.append((best, v, at))
                    (c, src, at), (x, xs, xat) = cand
                else:
                    c, src, at = inner[v2] * stay, v2, arg[v2]
                    x, xs, xat = inner[u] * p_switch, u, arg[u]
                if x > c or (variant == "voicing_tie_to_other" and x == c):
                    c, src, at = x, xs, xat
                new[v2, j] = (ov[j] if v2 else ou) * c
                back[t, v2, j] = (src, at)
        top = new.max()
        delta = new / top if top > 0.0 else new
    if variant == "per_frame_argmax":
        return (out, vp, delta) if detail else (out, vp)
    first = 1 if variant == "end_voiced_first" else 0
    v, m = first, 0
    for vv in (first, 1 - first):
        for i in range(M):
            if delta[vv, i] > delta[v, m]:
                v, m = vv, i
    for t in range(F - 1, -1, -1):
        if v:
            out[t] = centre[m]
            top, found = 0.0, False
            for c, b in enumerate(bins_of[t]):
                if b == m and (not found or prob[t, c] > top or (variant == "last_equal_candidate" and prob[t, c] == top)):
                    found, top, out[t] = True, prob[t, c], f0[t, c]
        v, m = back[t, v, m]
    return (out, vp, delta) if detail else (out, vp)


def track(x, tab, *, p_switch=0.01, p_absent=0.01, variant=None, **grid):
    """The chain of both stages for one wave: (f0 [F], voiced_prob [F]).  grid: first_centre, frames, window, hop, sample_rate."""
    count, _, f0, prob = candidates(x, w=tab["w"], p_absent=p_absent, tau_min=tab["tau_min"], tau_max=tab["tau_max"], variant=variant, **grid)
    return decode(count, f0, prob, edge=tab["edge"], centre=tab["centre"], reach=tab["reach"], trans=tab["trans"], p_switch=p_switch,
                  variant=variant)


# ---------------------------------------------------------------------------------------------------- fixtures
def octave_fixture(seed=3, seconds=0.45):
    """A 440 Hz five-harmonic tone with a Gaussian burst of the subharmonic in the middle: raw YIN reports 220 Hz on a few frames."""
    n = int(seconds * SR)
    g = np.random.default_rng(seed)
    phase = 2 * np.pi * 440.0 * np.arange(n) / SR
    x = np.zeros(n)
    for h in range(1, 6):
        x += np.sin(h * phase + g.uniform(0, 2 * np.pi)) / h
    burst = 1.1 * np.exp(-0.5 * ((np.arange(n) - n / 2) / (1.2 * HOP)) ** 2)
    return (0.3 * (x + burst * np.sin(phase / 2))).astype(np.float32)


def waves():
    """name -> f32 wave at the tests' shapes (43 to 60 frames of hop 256)."""
    n = int(0.45 * SR)
    return dict(octave=octave_fixture(), noise=Y.noise(0.45, seed=4), silence=np.zeros(n, np.float32),
                glide=Y.harmonic(np.linspace(160.0, 420.0, n), 0.45, seed=5), low=Y.harmonic(158.0, 0.45, seed=6),
                square=Y.square(150.0, 0.45), onset=np.concatenate([np.zeros(n // 2, np.float32), Y.harmonic(300.0, 0.3, seed=7)]))


@functools.lru_cache(maxsize=None)
def reference(name, first_centre=0, p_absent=0.01):
    """The oracle on one of waves() at the tests' shapes, computed once: (frames, (count, lag, f0, prob), (f0, voiced_prob))."""
    x, tab = waves()[name], tables()
    frames = len(x) // HOP + (1 if first_centre == 0 else 0)
    cand = candidates(x, w=tab["w"], p_absent=p_absent, first_centre=first_centre, frames=frames)
    out = decode(cand[0], cand[2], cand[3], edge=tab["edge"], centre=tab["centre"], reach=tab["reach"], trans=tab["trans"])
    return frames, cand, out


def inner(frames, n, first_centre=0):
    L = WINDOW + TAU_MAX + 1
    s0 = first_centre + np.arange(frames) * HOP - L // 2
    return (s0 >= 0) & (s0 + L <= n)


def bad_frames(f0, inn, target=440.0, cents=300.0):
    f0 = np.asarray(f0)[inn]
    with np.errstate(divide="ignore"):
        off = np.where(f0 > 0, np.abs(1200.0 * np.log2(np.where(f0 > 0, f0, 1.0) / target)), np.inf)
    return int((off > cents).sum())


def small_tables(M, reach, lo=100.0, ratio=2.0 ** (1 / 12)):
    """Geometric bins one semitone wide from `lo` Hz and a triangular, row-normalised band: for the hand-made cases."""
    edge = np.array([lo * ratio ** m for m in range(M + 1)])
    centre = np.array([lo * ratio ** (m + 0.5) for m in range(M)])
    trans = np.zeros((M, 2 * reach + 1))
    for i in range(M):
        for k in range(2 * reach + 1):
            if 0 <= i + k - reach < M:
                trans[i, k] = reach + 1 - abs(k - reach)
        trans[i] = trans[i] / math.fsum(trans[i])
    return dict(M=M, edge=edge, centre=centre, reach=reach, trans=trans)


def _table(rows, N):
    """rows: per frame a list of (f0, prob), given in ascending lag (descending f0) -> (count, f0 [F, N], prob [F, N])."""
    F = len(rows)
    count, f0, prob = np.zeros(F, np.int32), np.zeros((F, N)), np.zeros((F, N))
    for t, r in enumerate(rows):
        count[t] = len(r)
        for c, (f, p) in enumerate(r):
            f0[t, c], prob[t, c] = f, p
    return count, f0, prob


def decode_cases():
    """name -> (tables dict, (count, f0, prob), p_switch): the hand-made inputs of the decode."""
    out = {}
    t12 = small_tables(12, 3)
    c = t12["centre"]
    # a steady pitch with a two-frame octave-ish jump that the band (3 bins) cannot follow, an empty frame, a weak start
    rows = [[(c[4], 0.2)], [(c[4], 0.9)], [(c[5], 0.9)], [(c[11], 0.7), (c[5], 0.3)], [(c[11], 0.7), (c[4], 0.3)], [], [(c[4], 0.9)], [(c[3], 0.95)]]
    out["hand_made"] = (t12, _table(rows, 4), 0.01)
    # all-equal observations: every frame one candidate of the same prob in every bin -- the band's tie rule
    # decides (smallest source bin), and the end state's smallest bin; the voicing ties are "voicing_ties" below, the equal
    # candidates "equal_probs_in_a_bin", the edge rule "on_an_edge"
    t6 = small_tables(6, 2)
    flat = dict(t6, trans=np.where(t6["trans"] > 0, 0.25, 0.0))
    rows = [[(f, 0.125) for f in flat["centre"][::-1]] for _ in range(5)]
    out["all_equal"] = (flat, _table(rows, 8), 0.5)
    # the path must move by +reach and -reach, and flip its voicing in the same step as a full-reach move
    t9 = small_tables(9, 2)
    c = t9["centre"]
    rows = [[(c[2], 1.0)], [(c[4], 1.0)], [(c[6], 1.0)], [], [(c[4], 1.0)], [(c[2], 1.0)], [(c[0], 1.0)]]
    out["full_reach_and_flip"] = (t9, _table(rows, 2), 0.3)
    t2 = small_tables(2, 1)
    rows = [[(t2["centre"][0], 0.9)], [(t2["centre"][1], 0.8)], [], [(t2["centre"][1], 0.6), (t2["centre"][0], 0.4)]]
    out["two_bins"] = (t2, _table(rows, 2), 0.01)
    t512 = small_tables(512, 63, lo=50.0, ratio=2.0 ** (1 / 96))
    g = np.random.default_rng(11)
    walk = np.clip(200 + np.cumsum(g.integers(-40, 41, 12)), 0, 511)
    rows = [[(t512["centre"][m], 0.8)] + ([(t512["centre"][max(m - 96, 0)], 0.2)] if m >= 96 else []) for m in walk]
    out["many_bins"] = (t512, _table(rows, 3), 0.01)
    t5 = small_tables(5, 7)                                       # reach >= M: the band is every bin
    c = t5["centre"]
    rows = [[(c[0], 0.9)], [(c[4], 0.9)], [(c[1], 0.5), (c[0], 0.5)], [(c[3], 0.9)]]
    out["reach_over_bins"] = (t5, _table(rows, 2), 0.01)
    out["one_frame"] = (t12, _table([[(t12["centre"][7], 0.6), (t12["centre"][2], 0.3)]], 3), 0.01)
    out["no_candidates"] = (t12, _table([[], [], []], 2), 0.01)
    # tot rounds above 1: ten times 0.1 and one more ulp-sized vote; the unvoiced side sits on the floor
    rows = [[(t12["centre"][6], 0.1)] * 10 + [(t12["centre"][5], 2.0 ** -50)] for _ in range(3)]
    rows[1] = [(t12["centre"][6], 0.7), (t12["centre"][6], 0.3), (t12["centre"][6], 2.0 ** -52)]
    out["tot_over_one"] = (t12, _table(rows, 11), 0.01)
    # a jump the band cannot follow with no unvoiced escape: without the floor every delta is 0 from there on
    rows = [[(c12, 1.0)] for c12 in (t12["centre"][1], t12["centre"][1], t12["centre"][10], t12["centre"][10], t12["centre"][10])]
    out["unreachable_jump"] = (t12, _table(rows, 1), 0.01)
    # two steady paths, one in an edge bin whose row has fewer destinations (self-transition 0.4) and one inside (0.25): which one
    # wins depends on the rows being normalised
    rows = [[(t12["centre"][5], 0.6), (t12["centre"][0], 0.4)] for _ in range(6)]
    out["edge_rows"] = (t12, _table(rows, 2), 0.01)
    # probabilities from a coarse grid against thirds in the band: paths whose products tie or nearly tie, so that the order of the
    # two multiplications of the recurrence decides (found by search: the variant voicing_then_band decodes another path)
    t5b = small_tables(5, 2)
    g = np.random.default_rng(18)
    rows = [[(t5b["centre"][m], float(g.choice([0.1, 0.2, 0.3, 0.15]))) for m in range(4, -1, -1)] for _ in range(6)]
    out["near_ties"] = (t5b, _table(rows, 5), 0.3)
    # voicing ties in every frame, the last one included: two bins with 0.25 each, so ov = ou = 0.25, flat transitions and
    # p_switch = 0.5 -- delta(unvoiced, j) = delta(voiced, j) throughout.  The contract keeps the voicing and ends unvoiced.
    flat2 = dict(t2, trans=np.where(t2["trans"] > 0, 0.5, 0.0))
    rows = [[(t2["centre"][1], 0.25), (t2["centre"][0], 0.25)] for _ in range(4)]
    out["voicing_ties"] = (flat2, _table(rows, 2), 0.5)
    # two candidates of one bin with equal prob and different f0: the first in array order is the output
    c4 = t12["centre"][4]
    rows = [[(c4 * 1.01, 0.4), (c4 * 0.99, 0.4)] for _ in range(3)]
    out["equal_probs_in_a_bin"] = (t12, _table(rows, 2), 0.01)
    # a candidate exactly on edge[5] belongs to bin 5 (edge[j] <= f0): with it bin 5 holds 0.65 against 0.3 in bin 4; one bin
    # down, bin 4 would hold 0.6 against 0.35
    rows = [[(t12["centre"][5], 0.35), (t12["edge"][5], 0.3), (t12["centre"][4], 0.3)] for _ in range(3)]
    out["on_an_edge"] = (t12, _table(rows, 3), 0.01)
    return out
