"""What clipping a batch of raw prompts costs on the host, item by item, against the passes on the device.

  host    per prompt, vectorised numpy: the 16-bit view, one cumulative sum of the squares, every window's energy as a difference
          of two of its entries, the flags by the integer rule of include/f5_hip.h; the ranges through silence.py (the same host
          plan the device variant runs -- it is part of both); the clipped signal by numpy concatenation, analysed again the same
          way; then the ONE concatenated host-to-device copy of the results
  device  infer.clip_prompts(audios, rates): one concatenated copy of the RAW audio, f5_silence_analyse twice (a third time for the
          prompts whose grid shifts), two small reads of flags, f5_wave_gather; the clipped prompts stay on the device

on 32 synthetic prompts of 8 to 25 s that start on the host: bursts of noise at amplitude 0.1 between pauses of 0.15 to 1.6 s of
room noise, at 16, 22.05, 24, 44.1 and 48 kHz, mono and stereo.  pydub is not installed and is not what is compared here.

Both variants run in this process, alternating, each repetition inside a wall clock that ends in a device synchronise; the medians
of --reps repetitions after --warmup untimed ones are printed in milliseconds, as one JSON line.  Before timing, every prompt of the
device variant is compared bit for bit with the host variant's.

    python tools/silence_time.py [--reps 30] [--warmup 5]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from f5_tts_amd import infer as I  # noqa: E402
from f5_tts_amd import silence as S  # noqa: E402

DEV = "cuda:0"
RATES = (24000, 44100, 48000, 16000, 22050)
ITEMS = 32


def make_prompt(k: int):
    rng = np.random.default_rng(1000 + k)
    rate, channels = RATES[k % len(RATES)], 1 + (k // len(RATES)) % 2
    seconds = 8.0 + 17.0 * (k / (ITEMS - 1))
    parts, t = [], 0.0
    while t < seconds:
        burst, pause = rng.uniform(0.5, 3.0), rng.uniform(0.15, 1.6)
        parts.append(rng.standard_normal((channels, int(burst * rate))) * 0.1)
        parts.append(rng.standard_normal((channels, int(pause * rate))) * 0.0003)
        t += burst + pause
    x = np.concatenate(parts, axis=1)[:, :int(seconds * rate)].astype(np.float32)
    return torch.from_numpy(np.ascontiguousarray(x)), rate


def host_flags(prefix, frames, channels, rate, L, query):
    """The flags of one query from the frame-wise prefix sums of the squares (prefix[f] = sum over frames < f)."""
    W, s, T, kind = query
    starts = np.asarray(S.query_starts(L, W, s, kind), dtype=np.int64)
    ends = np.minimum(starts + W, L)
    fa, fb = starts * rate // 1000, ends * rate // 1000
    energy = prefix[np.minimum(fb, frames)] - prefix[np.minimum(fa, frames)]
    return energy < channels * (fb - fa) * (T + 1) ** 2


def host_prefix(q):
    return np.concatenate([[0], np.cumsum((q.astype(np.int64) ** 2).sum(axis=0))])


def host_signal(pieces, q):
    cols = [q[:, src:src + n] if src >= 0 else np.zeros((q.shape[0], n), dtype=q.dtype) for src, n in pieces]
    cols = [np.pad(c, ((0, 0), (0, n - c.shape[1]))) for c, (_, n) in zip(cols, pieces)]
    return np.concatenate(cols, axis=1) if cols else np.zeros((q.shape[0], 0), dtype=q.dtype)


def host_clip(x: np.ndarray, rate: int) -> np.ndarray:
    channels, frames = x.shape
    q = np.clip(np.rint(np.nan_to_num(x * np.float32(32768.0))), -32768, 32767).astype(np.int16)
    L = S.ms_len(frames, rate)
    prefix = host_prefix(q)
    pieces, _ = S.prompt_clip_plan(host_flags(prefix, frames, channels, rate, L, S.CLIP_QUERIES[0]),
                                   host_flags(prefix, frames, channels, rate, L, S.CLIP_QUERIES[1]), frames, rate)
    sig = host_signal(pieces, q)
    Ls = S.ms_len(sig.shape[1], rate)
    lead = S.leading_trim(host_flags(host_prefix(sig), sig.shape[1], channels, rate, Ls, S.EDGE_QUERIES[0]), Ls)
    rest, _ = S.after_lead(pieces, rate, lead)
    rsig = host_signal(rest, q)
    ms_flags = host_flags(host_prefix(rsig), rsig.shape[1], channels, rate, S.ms_len(rsig.shape[1], rate), S.EDGE_QUERIES[1])
    final, _ = S.finish_prompt(rest, S.trailing_cut(ms_flags, rsig.shape[1], rate), rate)
    return host_signal(final, q).astype(np.float32) / np.float32(32768.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if args.reps < 1 or args.warmup < 1:
        ap.error("--reps and --warmup must be >= 1")
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool only measures on the device")
    prompts = [make_prompt(k) for k in range(ITEMS)]
    audios, rates = [a for a, _ in prompts], [r for _, r in prompts]
    arrays = [a.numpy() for a in audios]

    def host():
        clipped = [host_clip(x, r) for x, r in zip(arrays, rates)]
        down = torch.from_numpy(np.concatenate([c.reshape(-1) for c in clipped])).to(DEV)
        return [p.view(c.shape) for p, c in zip(down.split([c.size for c in clipped]), clipped)]

    def device():
        return I.clip_prompts(audios, rates, device=DEV)[0]

    variants = {"host": host, "device": device}
    for _ in range(args.warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    hw, dw = host(), device()
    for k, (h, d) in enumerate(zip(hw, dw)):
        assert h.shape == d.shape and torch.equal(h.view(torch.int32), d.view(torch.int32)), f"prompt {k}: the device and the host disagree"
    wall = {k: [] for k in variants}
    for _ in range(args.reps):
        for k, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            wall[k].append((time.perf_counter() - t0) * 1e3)
    seconds_in = sum(a.shape[1] / r for a, r in prompts)
    seconds_out = sum(d.shape[1] / r for d, r in zip(dw, rates))
    rec = {"items": ITEMS, "audio_seconds_in": round(seconds_in, 1), "audio_seconds_out": round(seconds_out, 1),
           "input_mib": round(sum(a.numel() for a in audios) * 4 / 2 ** 20, 1), "reps": args.reps,
           "host_wall_ms_median": round(statistics.median(wall["host"]), 3),
           "device_wall_ms_median": round(statistics.median(wall["device"]), 3),
           "host_wall_ms_min_max": [round(min(wall["host"]), 3), round(max(wall["host"]), 3)],
           "device_wall_ms_min_max": [round(min(wall["device"]), 3), round(max(wall["device"]), 3)],
           "bit_equal_items": ITEMS}
    rec["host_over_device_wall"] = round(rec["host_wall_ms_median"] / rec["device_wall_ms_median"], 2)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
