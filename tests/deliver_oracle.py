"""The contract of f5_wave_deliver (include/f5_hip.h) as a numpy fold, for the tests: the rate geometry, the plan (len, ready), one
output sample at a time as the contract writes it -- taps ascending from +0.0, an f32 multiply then an f32 add per tap; numpy
rounds every f32 operation and fuses none -- and the 16-bit view.  The fold runs over the taps with all requested samples side by
side, which is the same arithmetic per sample.  The bank is the f32 cast of the float64 windowed-sinc kernel the product hands
its handle (mel.resample_kernel): an input of the contract, not part of what is checked here."""
import math

import numpy as np
import torch

STREAM_RATE = 24000


def geometry(out_rate):
    """(orig, new, width, K)."""
    g = math.gcd(STREAM_RATE, out_rate)
    orig, new = STREAM_RATE // g, out_rate // g
    if orig == new:
        return 1, 1, 0, 1
    width = math.ceil(6 * orig / (0.99 * min(orig, new)))
    return orig, new, width, 2 * width + orig


def plan(out_rate, n, final):
    """(len, ready) by the issue's formula."""
    orig, new, width, _ = geometry(out_rate)
    ln = -(-new * n // orig)
    if final:
        return ln, ln
    return ln, min(new * max(0, (n - width - orig) // orig + 1), ln)


def ready_by_count(out_rate, n):
    """ready of an unfinished stream by brute force: the leading outputs whose last tap lies inside the n samples."""
    orig, new, width, K = geometry(out_rate)
    ln, count = -(-new * n // orig), 0
    while count < ln and (count // new) * orig - width + K - 1 <= n - 1:
        count += 1
    return count


def bank_of(out_rate):
    from f5_tts_amd import mel as M

    return M.resample_kernel(STREAM_RATE, out_rate)[0][:, 0].to(torch.float32).numpy()      # [new, K]


def resample(x, out_rate, o0, o1, final=True):
    """y[o0:o1) of the stream x (f32 numpy) at out_rate, f32."""
    x = np.asarray(x, dtype=np.float32)
    orig, new, width, K = geometry(out_rate)
    ln, ready = plan(out_rate, len(x), final)
    assert 0 <= o0 <= o1 <= ready, (o0, o1, ready)
    if orig == new:
        return x[o0:o1].copy()
    bank = bank_of(out_rate)
    assert bank.shape == (new, K)
    xpad = np.concatenate([np.zeros(width, np.float32), x, np.zeros(width + 2 * orig, np.float32)])
    o = np.arange(o0, o1)
    i, p = o // new, o % new
    acc = np.zeros(o1 - o0, np.float32)
    for k in range(K):
        acc = acc + bank[p, k] * xpad[i * orig + k]
    assert acc.dtype == np.float32
    return acc


def quantise(y):
    """F5_PCM_S16: t = y * 32767.f in f32; NaN -> 0, t <= -32768 -> -32768, t >= 32767 -> 32767, else rint (ties to even)."""
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.asarray(y, np.float32) * np.float32(32767.0)
        q = np.clip(np.rint(t), -32768.0, 32767.0)
    return np.where(np.isnan(t), 0.0, q).astype(np.int16)


def deliver(x, out_rate, sample_format="f32", final=True, o0=0, o1=None):
    if o1 is None:
        o1 = plan(out_rate, len(x), final)[1]
    y = resample(x, out_rate, o0, o1, final)
    return y if sample_format == "f32" else quantise(y)
