"""NumPy float64 oracles of the Gaussian cepstral divergence, written from the arithmetic contract in include/f5_hip.h (the section
"speaker similarity"), not from the kernels.

The ORDERED oracle (`moments`, `divergence`) follows the contract's order of operations: every sum that the contract orders is a
Python loop over the ordered index (mel bin, frame, chunk, k of a Cholesky or substitution chain); only indices the contract leaves
independent of one another (different entries, different rows) are NumPy-vectorised, which evaluates each element with the same single
IEEE operations.  The Cholesky factor and the substitutions are by hand; no LAPACK.
The PLAIN oracle (`plain_moments`, `plain_terms`) is np.cov and np.linalg: what the numbers mean, in no particular order.
`synthetic_speaker` / `synthetic_utterance` are the construction of the discrimination test."""
import math

import numpy as np

MOM_CHUNK = 64


def dct_table(n_mels: int, n_cep: int) -> np.ndarray:
    """T[j][k - 1], the contract's expression evaluated left to right with the C library's cosine (math.cos)."""
    norm = math.sqrt(2.0 / n_mels)
    T = np.empty((n_mels, n_cep), dtype=np.float64)
    for j in range(n_mels):
        for k in range(1, n_cep + 1):
            T[j, k - 1] = norm * math.cos(math.pi * k * (j + 0.5) / n_mels)
    return T


def features(x, n_cep: int, deltas: bool) -> np.ndarray:
    """The feature vectors [F, C] of one segment x [F, n_mels] (f32)."""
    x = np.asarray(x, dtype=np.float32)
    F, n_mels = x.shape
    T = dct_table(n_mels, n_cep)
    c = np.zeros((F, n_cep), dtype=np.float64)
    for j in range(n_mels):                         # j ascending: multiply, then add
        c = c + x[:, j:j + 1].astype(np.float64) * T[j][None, :]
    if not deltas:
        return c
    t = np.arange(F)
    at = lambda o: c[np.clip(t + o, 0, F - 1)]      # noqa: E731
    d = ((at(1) - at(-1)) + 2.0 * (at(2) - at(-2))) / 10.0
    return np.concatenate([c, d], axis=1)


def energies(x) -> np.ndarray:
    x = np.asarray(x, dtype=np.float32)
    e = np.zeros(x.shape[0], dtype=np.float64)
    for j in range(x.shape[1]):
        e = e + x[:, j].astype(np.float64)
    return e


def selection(x, mask=None, gate_sum: float = -1.0):
    """(selected [F] bool, finite): the contract's selection for one segment; mask is the segment's own slice."""
    e = energies(x)
    if not np.all(np.isfinite(e)):
        return None, False
    sel = np.ones(e.shape[0], dtype=bool) if mask is None else np.asarray(mask).astype(bool).copy()
    if gate_sum >= 0:
        sel &= e >= (np.max(e) - gate_sum)
    return sel, True


def triu(C: int):
    return np.triu_indices(C)                       # row-major over the upper triangle


def moments(x, n_cep: int = 13, deltas: bool = False, mask=None, gate_sum: float = -1.0):
    """(count, mean [C], scatter [C (C + 1) / 2]) of one segment, in the contract's order."""
    C = n_cep * (2 if deltas else 1)
    p, q = triu(C)
    sel, finite = selection(x, mask, gate_sum)
    if not finite:
        return -1, np.full(C, np.nan), np.full(len(p), np.nan)
    v = features(x, n_cep, deltas)
    F = v.shape[0]
    n, total = 0, np.zeros(C)
    for lo in range(0, F, MOM_CHUNK):               # pass 1
        part = np.zeros(C)
        for t in range(lo, min(lo + MOM_CHUNK, F)):
            if sel[t]:
                part = part + v[t]
                n += 1
        total = total + part
    if n == 0:
        return 0, np.zeros(C), np.zeros(len(p))
    mean = total / float(n)
    scatter = np.zeros(len(p))
    for lo in range(0, F, MOM_CHUNK):               # pass 2
        part = np.zeros(len(p))
        for t in range(lo, min(lo + MOM_CHUNK, F)):
            if sel[t]:
                d = v[t] - mean
                part = part + d[p] * d[q]
        scatter = scatter + part
    return n, mean, scatter


def cholesky(A: np.ndarray):
    """(L, ok): the lower factor column by column; ok is False when a pivot is <= 0 or not finite."""
    C = A.shape[0]
    L = np.zeros((C, C))
    for c in range(C):
        s = A[c:, c].copy()                         # rows r >= c, independent of one another
        for k in range(c):
            s = s - L[c:, k] * L[c, k]
        piv = s[0]
        if not (piv > 0.0 and np.isfinite(piv)):
            return L, False
        L[c, c] = math.sqrt(piv)
        L[c + 1:, c] = s[1:] / L[c, c]
    return L, True


def solve_lower(L: np.ndarray, B: np.ndarray) -> np.ndarray:
    """L^-1 B for a lower-triangular B [C, C], column c down its rows r >= c with k = c .. r - 1 ascending."""
    C = L.shape[0]
    X = np.zeros((C, C))
    for c in range(C):
        for r in range(c, C):
            s = B[r, c]
            for k in range(c, r):
                s = s - L[r, k] * X[k, c]
            X[r, c] = s / L[r, r]
    return X


def solve_vector(L: np.ndarray, d: np.ndarray) -> np.ndarray:
    C = L.shape[0]
    z = np.zeros(C)
    for r in range(C):
        s = d[r]
        for k in range(r):
            s = s - L[r, k] * z[k]
        z[r] = s / L[r, r]
    return z


def frob2(X: np.ndarray) -> float:
    tr = 0.0
    for c in range(X.shape[0]):
        col = 0.0
        for r in range(c, X.shape[0]):
            col = col + X[r, c] * X[r, c]
        tr = tr + col
    return tr


def unpack(scatter: np.ndarray, C: int) -> np.ndarray:
    S = np.zeros((C, C))
    p, q = triu(C)
    S[p, q] = scatter
    S[q, p] = scatter
    return S


def divergence(rec_i, rec_j):
    """((tr_ij, tr_ji, q_i, q_j), status) of two records (count, mean, scatter), in the contract's order."""
    (ni, mi, si), (nj, mj, sj) = rec_i, rec_j
    C = len(mi)
    nan4 = (math.nan,) * 4
    if ni <= C or nj <= C:
        return nan4, 1
    Li, ok_i = cholesky(unpack(np.asarray(si) / float(ni), C))
    Lj, ok_j = cholesky(unpack(np.asarray(sj) / float(nj), C))
    if not (ok_i and ok_j):
        return nan4, 1
    d = np.asarray(mi) - np.asarray(mj)
    zi, zj = solve_vector(Li, d), solve_vector(Lj, d)
    q = lambda z: float(sum_ascending(z * z))       # noqa: E731
    return (frob2(solve_lower(Li, Lj)), frob2(solve_lower(Lj, Li)), q(zi), q(zj)), 0


def sum_ascending(values) -> float:
    acc = 0.0
    for v in values:
        acc = acc + v
    return acc


def numbers(terms, C: int):
    """(kl, sphericity) as metrics.speaker_numbers states them."""
    tr_ij, tr_ji, q_i, q_j = terms
    kl = 0.5 * ((tr_ij + tr_ji) - 2 * C) + 0.5 * (q_i + q_j)
    ratio = tr_ij * tr_ji / (C * C)
    return kl, (math.log(ratio) if ratio > 0 else math.nan)


def merge(rec_a, rec_b):
    """The pairwise update of two records."""
    (na, ma, sa), (nb, mb, sb) = rec_a, rec_b
    C = len(ma)
    p, q = triu(C)
    n = na + nb
    d = np.asarray(mb) - np.asarray(ma)
    return n, ma + d * (nb / n), sa + sb + d[p] * d[q] * (na * nb / n)


# ---------------------------------------------------------------------------------------------------- the plain oracle
def plain_features(x, n_cep: int, deltas: bool) -> np.ndarray:
    x = np.asarray(x, dtype=np.float64)
    n_mels = x.shape[1]
    k = np.arange(1, n_cep + 1, dtype=np.float64)[None, :]
    j = np.arange(n_mels, dtype=np.float64)[:, None]
    c = x @ (np.sqrt(2.0 / n_mels) * np.cos(np.pi * k * (j + 0.5) / n_mels))
    if not deltas:
        return c
    pad = np.concatenate([c[:1], c[:1], c, c[-1:], c[-1:]])
    d = (pad[3:-1] - pad[1:-3] + 2.0 * (pad[4:] - pad[:-4])) / 10.0
    return np.concatenate([c, d], axis=1)


def plain_moments(x, n_cep: int = 13, deltas: bool = False, sel=None):
    """(count, mean, covariance matrix with divisor n) by np.mean / np.cov."""
    v = plain_features(x, n_cep, deltas)
    if sel is not None:
        v = v[np.asarray(sel).astype(bool)]
    return v.shape[0], v.mean(axis=0), np.atleast_2d(np.cov(v, rowvar=False, bias=True))


def plain_terms(mean_i, cov_i, mean_j, cov_j):
    d = mean_i - mean_j
    return (float(np.trace(np.linalg.solve(cov_i, cov_j))), float(np.trace(np.linalg.solve(cov_j, cov_i))),
            float(d @ np.linalg.solve(cov_i, d)), float(d @ np.linalg.solve(cov_j, d)))


# ---------------------------------------------------------------------------------------------------- synthetic voices
def synthetic_speaker(rng, n_mels: int = 100, n_src: int = 8):
    """A speaker: a random smooth spectral envelope and a speaker-specific mixing of the shared content process into the mel bins."""
    j = np.arange(n_mels) / n_mels
    env = sum(rng.normal() * np.cos(np.pi * h * j) / h for h in range(1, 6)) * 2.0 - 6.0
    width = rng.uniform(0.04, 0.12, n_src)
    centre = rng.uniform(0.0, 1.0, n_src)
    mix = rng.uniform(0.5, 1.5, n_src)[:, None] * np.exp(-0.5 * ((j[None, :] - centre[:, None]) / width[:, None]) ** 2)
    return env, mix


def synthetic_utterance(rng, speaker, frames: int, rho: float = 0.9) -> np.ndarray:
    """frames of log-mel: the speaker's envelope plus its mixing of an AR(1) content process (the process's law is shared by all
    speakers; every utterance draws its own path), plus a little white noise."""
    env, mix = speaker
    n_src = mix.shape[0]
    z = np.zeros((frames, n_src))
    state = rng.normal(size=n_src)
    for t in range(frames):
        state = rho * state + math.sqrt(1.0 - rho * rho) * rng.normal(size=n_src)
        z[t] = state
    return (env[None, :] + z @ mix + 0.05 * rng.normal(size=(frames, mix.shape[1]))).astype(np.float32)
