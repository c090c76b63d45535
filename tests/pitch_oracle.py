"""The yardstick of the pitch-track tests: the contract of include/f5_hip.h (f5_pitch_track: YIN) restated in NumPy float64, sharing
no code with the package.  For frame t of a wave x (f32, len samples), W = window:

  samples      L = W + tau_max + 1, s0 = first_centre + t * hop - L // 2; sample s0 + j, 0 outside [0, len).
  difference   d(tau) = sum_{j < W} ((double)x[j] - (double)x[j + tau])^2, tau = 1 .. tau_max + 1, j ascending, multiply then add.
  cumulative   S(tau) = S(tau - 1) + d(tau), S(0) = 0, ascending.
  normalised   d'(tau) = (d(tau) * tau) / S(tau) if S(tau) > 0 else 1.
  choice       the smallest tau in [tau_min, tau_max] with d'(tau) < threshold, then on while tau + 1 <= tau_max and d'(tau + 1) <
               d'(tau); none: unvoiced, f0 = 0, ap = min d' over the range.
  refinement   a, b, c = d'(tau - 1), d'(tau), d'(tau + 1); den = a - 2 b + c; delta = 0.5 (a - c) / den if den > 0 else 0, clamped to
               [-0.5, 0.5]; f0 = sample_rate / (tau + delta), ap = b.

The sums run over j (and the cumulative sum over tau) in Python loops, vectorised only across frames and lags, which have no order.
It also carries named WRONG variants (VARIANTS): trackers a kernel could plausibly be instead.  s_with_d0 is "S including d(0)" as
the mean over the tau + 1 terms d(0) .. d(tau) (d(0) = 0 adds nothing to the sum itself): d' times (tau + 1) / tau."""
import math

import numpy as np

VARIANTS = ("raw_d", "no_descent", "no_parabola", "window_at_centre", "s_with_d0")


def lags(sample_rate, fmin=60.0, fmax=600.0):
    return int(math.floor(sample_rate / fmax)), int(math.ceil(sample_rate / fmin))


def frame_matrix(x, frames, hop, first_centre, L, at_centre=False):
    x = np.asarray(x, dtype=np.float32)
    s0 = first_centre + np.arange(frames)[:, None] * hop - (0 if at_centre else L // 2)
    idx = s0 + np.arange(L)[None, :]
    ok = (idx >= 0) & (idx < len(x))
    return np.where(ok, x[np.clip(idx, 0, len(x) - 1)], np.float32(0)).astype(np.float64)


def normalised_difference(X, W, tau_max, variant=None):
    """d' [frames, tau_max + 2] (column tau; column 0 unused) and the raw d."""
    F = X.shape[0]
    d = np.zeros((F, tau_max + 2), dtype=np.float64)
    for j in range(W):
        diff = X[:, j:j + 1] - X[:, j + 1:j + tau_max + 2]
        d[:, 1:] += diff * diff
    S = np.zeros(F, dtype=np.float64)
    dn = np.ones_like(d)
    for tau in range(1, tau_max + 2):
        S = S + d[:, tau]
        num = d[:, tau] * float(tau + 1 if variant == "s_with_d0" else tau)
        with np.errstate(divide="ignore", invalid="ignore"):
            dn[:, tau] = np.where(S > 0, num / S, 1.0)
    return dn, d


def track(x, *, sample_rate=24000, hop=256, first_centre=0, frames=None, window=1024, tau_min=40, tau_max=400, threshold=0.15,
          variant=None, detail=False):
    """(f0, ap) float64 [frames] under the contract (variant None) or one of the named wrong VARIANTS.  detail=True adds the smallest
    distance from equality of every comparison that decided something: (|d' - threshold| over the scanned lags, |d'(tau+1) - d'(tau)|
    over the descent steps)."""
    assert variant is None or variant in VARIANTS, variant
    x = np.asarray(x, dtype=np.float32)
    frames = len(x) // hop + 1 if frames is None else frames
    L = window + tau_max + 1
    X = frame_matrix(x, frames, hop, first_centre, L, at_centre=variant == "window_at_centre")
    dn, d = normalised_difference(X, window, tau_max, variant)
    if variant == "raw_d":
        dn = d
    f0, ap = np.zeros(frames), np.zeros(frames)
    gap_thr, gap_desc = np.inf, np.inf
    for t in range(frames):
        row = dn[t]
        tau = 0
        for k in range(tau_min, tau_max + 1):
            gap_thr = min(gap_thr, abs(row[k] - threshold))
            if row[k] < threshold:
                tau = k
                break
        if not tau:
            m = row[tau_min]
            for k in range(tau_min + 1, tau_max + 1):
                if row[k] < m:
                    m = row[k]
            f0[t], ap[t] = 0.0, m
            continue
        if variant != "no_descent":
            while tau + 1 <= tau_max:
                gap_desc = min(gap_desc, abs(row[tau + 1] - row[tau]))
                if not row[tau + 1] < row[tau]:
                    break
                tau += 1
        a, b, c = row[tau - 1], row[tau], row[tau + 1]
        den = a - 2.0 * b + c
        delta = (0.5 * (a - c)) / den if den > 0 else 0.0
        delta = -0.5 if delta < -0.5 else (0.5 if delta > 0.5 else delta)
        if variant == "no_parabola":
            delta = 0.0
        f0[t], ap[t] = float(sample_rate) / (float(tau) + delta), b
    return (f0, ap, gap_thr, gap_desc) if detail else (f0, ap)


# ---------------------------------------------------------------------------------------------------- fixtures
TONES = (65, 80, 110, 155, 220, 311, 440, 523, 590)


def harmonic(freq, seconds=0.5, sample_rate=24000, seed=0, harmonics=5):
    """Five harmonics at amplitude 1 / h with random phases; freq a number or an array of instantaneous frequencies."""
    g = np.random.default_rng(seed)
    n = int(seconds * sample_rate)
    f = np.broadcast_to(np.asarray(freq, dtype=np.float64), (n,))
    phase = 2 * np.pi * np.cumsum(f) / sample_rate
    x = np.zeros(n)
    for h in range(1, harmonics + 1):
        x += np.sin(h * phase + g.uniform(0, 2 * np.pi)) / h
    return (0.3 * x).astype(np.float32)


def glide(f_lo=100.0, f_hi=300.0, seconds=0.5, sample_rate=24000, seed=0):
    n = int(seconds * sample_rate)
    return harmonic(np.linspace(f_lo, f_hi, n), seconds, sample_rate, seed), np.linspace(f_lo, f_hi, n)


def noise(seconds=0.5, sample_rate=24000, seed=0):
    return (0.3 * np.random.default_rng(seed).standard_normal(int(seconds * sample_rate))).astype(np.float32)


def square(freq=150.0, seconds=0.5, sample_rate=24000):
    """A +-1 square wave with a whole number of samples per period: exact ties in d'."""
    period = int(round(sample_rate / freq))
    n = int(seconds * sample_rate)
    return np.where(np.arange(n) % period < period // 2, 1.0, -1.0).astype(np.float32)


def inner(frames, hop=256, window=1024, tau_max=400, n=None):
    """The frames whose L samples lie wholly inside the wave (first_centre = 0)."""
    L = window + tau_max + 1
    t = np.arange(frames)
    s0 = t * hop - L // 2
    return (s0 >= 0) & (s0 + L <= n)
