"""The yardstick of the mel-distance tests: the contract of include/f5_hip.h (DTW-aligned mel-cepstral distance) restated in NumPy
float64, sharing no code with the package.  Cepstra by a loop over the mel bins, the frame distances as a matrix, D by vectorised
anti-diagonals.  For a pair (a [n, n_mels], b [m, n_mels]) of natural-log mels:

  cepstra    c_k(x) = sum_j (double)x_j * T[k][j], k = 1 .. n_cep, T[k][j] = sqrt(2 / n_mels) cos(pi k (j + 0.5) / n_mels), j ascending,
             multiply then add: the orthonormal DCT-II without coefficient 0.
  distance   d(i, j) = SCALE * sqrt(2 * sum_k (c_k(a_i) - c_k(b_j))^2), k ascending, SCALE the double 10 / ln 10.
  alignment  D(0, 0) = 2 d(0, 0); D(i, j) = min(D(i-1, j) + d, D(i-1, j-1) + 2 d, D(i, j-1) + d), +inf outside the grid.
  value      D(n-1, m-1) / (n + m): every path has total weight n + m.

It also carries named WRONG variants (VARIANTS): recurrences and distances a kernel could plausibly compute instead.  The CPU test
holds every one of them at least 1e-3 (relative) away from the true value on the fixtures, so the GPU gate cannot hide one."""
import numpy as np

SCALE = 4.3429448190325175          # 10 / ln 10
assert SCALE == 10.0 / np.log(10.0)

VARIANTS = ("diag_weight_1", "path_length", "with_c0", "squared", "init_d", "asymmetric")


def dct_table(n_mels: int, n_cep: int, first: int = 1) -> np.ndarray:
    """T[k - first][j] for k = first .. first + n_cep - 1 (coefficient 0, where asked for, with its orthonormal factor)."""
    k = np.arange(first, first + n_cep, dtype=np.float64)[:, None]
    j = np.arange(n_mels, dtype=np.float64)[None, :]
    T = np.sqrt(2.0 / n_mels) * np.cos(np.pi * k * (j + 0.5) / n_mels)
    if first == 0:
        T[0] = np.sqrt(1.0 / n_mels)
    return T


def cepstra(x, n_cep: int, first: int = 1) -> np.ndarray:
    x = np.asarray(x, dtype=np.float32)
    T = dct_table(x.shape[1], n_cep, first)
    c = np.zeros((x.shape[0], n_cep), dtype=np.float64)
    for j in range(x.shape[1]):
        c += x[:, j:j + 1].astype(np.float64) * T[None, :, j]
    return c


def frame_distances(ca: np.ndarray, cb: np.ndarray, squared: bool = False) -> np.ndarray:
    acc = np.zeros((ca.shape[0], cb.shape[0]), dtype=np.float64)
    for k in range(ca.shape[1]):
        diff = ca[:, k][:, None] - cb[:, k][None, :]
        acc += diff * diff
    return SCALE * (2.0 * acc) if squared else SCALE * np.sqrt(2.0 * acc)


def accumulate(d: np.ndarray, *, w_diag: float = 2.0, w_init: float = 2.0, w_left: float = 1.0, full: bool = False):
    """D(n-1, m-1) of the recurrence over the anti-diagonals s = i + j; full=True returns the whole matrix D instead."""
    n, m = d.shape
    # a diagonal as an array over i + 1 (slot 0 is i = -1): +inf wherever (i, s - i) is outside the grid
    prev1 = np.full(n + 1, np.inf)
    prev2 = np.full(n + 1, np.inf)
    D = np.full((n, m), np.inf) if full else None
    for s in range(n + m - 1):
        i = np.arange(max(0, s - m + 1), min(n - 1, s) + 1)
        dd = d[i, s - i]
        cur = np.full(n + 1, np.inf)
        if s == 0:
            cur[1] = w_init * dd[0]
        else:
            up, left, diag = prev1[i], prev1[i + 1], prev2[i]
            cur[i + 1] = np.minimum(np.minimum(up + dd, diag + w_diag * dd), left + w_left * dd)
        if full:
            D[i, s - i] = cur[i + 1]
        prev2, prev1 = prev1, cur
    return D if full else prev1[n]


def _path_cells(D: np.ndarray) -> int:
    """The number of cells of one optimal path, by backtracking to the smallest predecessor (the diagonal first on ties)."""
    i, j, cells = D.shape[0] - 1, D.shape[1] - 1, 1
    while i > 0 or j > 0:
        cand = [(D[i - 1, j - 1] if i > 0 and j > 0 else np.inf, i - 1, j - 1), (D[i - 1, j] if i > 0 else np.inf, i - 1, j),
                (D[i, j - 1] if j > 0 else np.inf, i, j - 1)]
        _, i, j = min(cand, key=lambda c: c[0])
        cells += 1
    return cells


def value(a, b, n_cep: int = 13, variant: str | None = None) -> float:
    """The pair's value under the contract (variant None), or under one of the named wrong VARIANTS."""
    assert variant is None or variant in VARIANTS, variant
    n, m = len(a), len(b)
    if variant == "with_c0":
        ca, cb = cepstra(a, n_cep + 1, first=0), cepstra(b, n_cep + 1, first=0)
    else:
        ca, cb = cepstra(a, n_cep), cepstra(b, n_cep)
    d = frame_distances(ca, cb, squared=variant == "squared")
    if variant == "diag_weight_1":
        return accumulate(d, w_diag=1.0) / (n + m)
    if variant == "init_d":
        return accumulate(d, w_init=1.0) / (n + m)
    if variant == "asymmetric":                      # the horizontal step is free, normalised by the rows alone
        return accumulate(d, w_diag=1.0, w_init=1.0, w_left=0.0) / n
    if variant == "path_length":
        D = accumulate(d, full=True)
        return D[-1, -1] / _path_cells(D)
    return accumulate(d) / (n + m)


# ---------------------------------------------------------------------------------------------------- fixtures
def random_walk_mel(seed: int, frames: int, n_mels: int = 100) -> np.ndarray:
    """A smooth log-mel: a random walk in time of a smooth spectral envelope, f32 [frames, n_mels], in natural-log units (about -11 .. 2)."""
    g = np.random.default_rng(seed)
    steps = g.standard_normal((frames, 8)) * 0.25
    steps[0] = g.standard_normal(8) * 1.5
    coef = np.cumsum(steps, axis=0)
    basis = np.cos(np.pi * np.arange(8)[:, None] * (np.arange(n_mels)[None, :] + 0.5) / n_mels) / (1.0 + np.arange(8)[:, None])
    return (coef @ basis - 4.0).astype(np.float32)


def warped(a: np.ndarray, seed: int, frames: int, noise: float = 0.05) -> np.ndarray:
    """`a` resampled in time onto `frames` frames along a smooth monotone warp (linear interpolation), plus white noise."""
    g = np.random.default_rng(seed)
    u = np.linspace(0.0, 1.0, frames)
    w = u + 0.08 * g.uniform(-1, 1) * np.sin(np.pi * u) + 0.04 * g.uniform(-1, 1) * np.sin(2 * np.pi * u)
    pos = np.clip(w, 0.0, 1.0) * (len(a) - 1)
    lo = np.floor(pos).astype(int)
    hi = np.minimum(lo + 1, len(a) - 1)
    frac = (pos - lo)[:, None]
    out = (1.0 - frac) * a[lo].astype(np.float64) + frac * a[hi].astype(np.float64)
    return (out + noise * g.standard_normal(out.shape)).astype(np.float32)


def pair(seed: int, n: int, m: int, n_mels: int = 100):
    a = random_walk_mel(seed, n, n_mels)
    return a, warped(a, seed + 1000, m)
