"""The yardstick of the alignment and prosody tests: dtw_oracle.py's D with back-pointers under the tie rule of include/f5_hip.h
(f5_mel_align), and the fold of two pitch tracks along a path, in NumPy float64 and plain Python loops.

  predecessor  of (i, j): the candidate with the smallest sum among D(i-1, j-1) + 2 d(i, j), D(i-1, j) + d(i, j), D(i, j-1) + d(i, j);
               on equal sums the diagonal first, then (i-1, j), then (i, j-1).  The path is the chain from (n-1, m-1) to (0, 0),
               reported forward."""
import math

import numpy as np

import dtw_oracle as O

# (n, m) of the random-fixture alignment cases, one device call per group, shared by the CPU test (which holds their smallest gap
# between competing candidates above the GPU test's premise) and the GPU test: the smallest pairs, the wave (64), the workgroup's
# column count (256: the strip goes from 1 to 2), 512 / 513, strip 16, the ring wrap and the side swap.
ALIGN_CASES = {
    "edges": [(1, 1), (1, 7), (7, 1), (2, 2), (3, 129)],
    "wave": [(70, 63), (70, 64), (70, 65), (63, 70), (64, 64), (65, 65)],
    "workgroup_columns": [(300, 255), (300, 256), (300, 257), (257, 300), (256, 256)],
    "two_strips": [(520, 512), (520, 513), (513, 513)],
    "strip_16": [(2049, 2100)],
    "ring_and_swap": [(700, 90), (90, 700)],
}
ALL_TIE = [(5, 9), (9, 5), (300, 260)]


# The fixture of a case is O.pair(seed, n, m), the seed 7000 + 131 k + n + 3 m (k: the case's place in its group) plus 1000 times the
# step below: the first step at which the smallest non-zero relative gap between competing candidates exceeds 2^-39 at n_cep = 1 and
# at n_cep = 13, found with this module alone.  A gap of one ulp is no flaw of a kernel: with one coefficient d(i, j) is
# c |x_i - y_j|, and paths that visit every row and column equally often over a patch of constant sign cost the same in exact
# arithmetic; the chance of one such pair of paths grows with the grid (five of twelve seeds tried at 300 x 255, eight of twelve at 520 x 513).
SEED_STEPS = {(300, 255): 1, (300, 257): 1, (256, 256): 1, (520, 513): 5, (513, 513): 5, (700, 90): 2}
# (group, n, m, n_cep) -> the measured gap where NO fixture was found: 60 seeds of O.pair, six with noise 1.0 and four of white noise
# all measure 1.1e-16 .. 1.2e-16 on this grid of 4.3 M cells.  There the GPU test has the value bit-equal to the oracle's instead.
GAP_EXCEPTIONS = {("strip_16", 2049, 2100, 1): 1.2e-16}


def case_pairs(group, n_mels=100):
    return [O.pair(7000 + 131 * k + n + 3 * m + 1000 * SEED_STEPS.get((n, m), 0), n, m, n_mels)
            for k, (n, m) in enumerate(ALIGN_CASES[group])]


def candidates(D, d):
    """The three sums of every cell, [3, n, m] in the rule's order, +inf where the predecessor is outside the grid."""
    n, m = d.shape
    pad = np.full((n + 1, m + 1), np.inf)
    pad[1:, 1:] = D
    return np.stack([pad[:-1, :-1] + 2.0 * d, pad[:-1, 1:] + d, pad[1:, :-1] + d])


def path_of(D, d, detail=False):
    """The path [(i, j), ...] forward from (0, 0); detail=True adds the smallest non-zero relative gap between the best and any
    other candidate over ALL cells (what a last-bit difference in D would have to bridge to flip a choice)."""
    n, m = d.shape
    cand = candidates(D, d)
    code = np.argmin(cand, axis=0)                  # the first of the smallest: the rule's order
    i, j, cells = n - 1, m - 1, [(n - 1, m - 1)]
    while i > 0 or j > 0:
        c = code[i, j]
        i, j = (i - 1, j - 1) if c == 0 else ((i - 1, j) if c == 1 else (i, j - 1))
        cells.append((i, j))
    cells.reverse()
    if not detail:
        return cells
    best = cand.min(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = (cand - best[None]) / best[None]
    rel = rel[np.isfinite(rel) & (rel > 0)]
    return cells, (rel.min() if rel.size else np.inf)


def alignment(a, b, n_cep=13, detail=False):
    """(value, path) of a pair of mels, as f5_mel_align defines them."""
    d = O.frame_distances(O.cepstra(a, n_cep), O.cepstra(b, n_cep))
    D = O.accumulate(d, full=True)
    out = path_of(D, d, detail)
    value = D[-1, -1] / (len(a) + len(b))
    return (value,) + out if detail else (value, out)


def all_paths(n, m):
    """Every monotone path from (0, 0) to (n-1, m-1) with steps (1, 0), (1, 1), (0, 1)."""
    def go(i, j):
        if (i, j) == (n - 1, m - 1):
            yield [(i, j)]
            return
        for di, dj in ((1, 1), (1, 0), (0, 1)):
            if i + di < n and j + dj < m:
                for rest in go(i + di, j + dj):
                    yield [(i, j)] + rest
    return list(go(0, 0))


def path_cost(path, d):
    """w * d folded along the path in forward order: 2 d(0, 0), then d or 2 d (diagonal) per step."""
    total = 2.0 * d[0, 0]
    for (pi, pj), (i, j) in zip(path, path[1:]):
        total = total + (2.0 if (i - pi, j - pj) == (1, 1) else 1.0) * d[i, j]
    return total


def path_weight(path):
    return 2 + sum(2 if (i - pi, j - pj) == (1, 1) else 1 for (pi, pj), (i, j) in zip(path, path[1:]))


SUMS = ("diff", "diff2", "x", "y", "xy", "x2", "y2")


def fold(f0_a, f0_b, path):
    """The per-cell loop: counts and the sums over the cells voiced on both sides, x = log2 f0_a, y = log2 f0_b."""
    out = dict(cells=0, both_voiced=0, vuv_mismatch=0, **{k: 0.0 for k in SUMS})
    for i, j in path:
        fa, fb = float(f0_a[i]), float(f0_b[j])
        out["cells"] += 1
        if (fa > 0) != (fb > 0):
            out["vuv_mismatch"] += 1
        if fa > 0 and fb > 0:
            x, y = math.log2(fa), math.log2(fb)
            out["both_voiced"] += 1
            for k, v in zip(SUMS, (x - y, (x - y) * (x - y), x, y, x * y, x * x, y * y)):
                out[k] += v
    return out
