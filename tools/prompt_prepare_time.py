"""What preparing a batch of raw prompts costs on the host, item by item, against one pass on the device.

  host    [infer.normalise_prompt(a, sr) for each prompt] (mono mix, RMS, gain, sinc_resample: torch on the CPU), then the ONE
          concatenated host-to-device copy MelSpec.forward_ragged makes of the results
  device  MelSpec.prepare_ragged(audios, rates): one concatenated copy of the RAW audio, then f5_mel_prepare_ragged (three
          launches and one table copy); the waveforms and the rms stay on the device

on prompts that start on the host (random samples at amplitude 0.05, so every item is levelled; the cost does not depend on them):

  a  64 prompts of 10 s, stereo, 44.1 kHz
  b  64 prompts of 10 s, mono, 48 kHz
  c   1 prompt  of 10 s, stereo, 44.1 kHz

Both variants run in this process, alternating, each repetition between two events on the stream and inside a wall clock that ends
in a device synchronise; the medians of --reps repetitions after --warmup untimed ones are printed in milliseconds.  The stream
is idle when a repetition starts, so both figures of the host variant contain its CPU work.  The device results are checked
against the host's under the forward error bound of an f32 recursive sum, (K + 1) * 2^-24 * sum_k |bank[p][k] * v[i * orig + k]| per sample (in
float64, for the first and the last item; both sides are within it of the float64 result, so they are within twice it of each
other), and the rms against the host's.

    python tools/prompt_prepare_time.py [--reps 30] [--warmup 5]
    rocprofv3 --kernel-trace --stats -- python tools/prompt_prepare_time.py --reps 3 --warmup 1     # per-kernel times, own run
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import f5_tts_amd as P  # noqa: E402
from f5_tts_amd import infer as I  # noqa: E402
from f5_tts_amd.mel import resample_kernel  # noqa: E402

DEV = "cuda:0"
TARGET, TARGET_RMS = 24000, 0.1
SHAPES = {"a": (64, 2, 44100), "b": (64, 1, 48000), "c": (1, 2, 44100)}
SECONDS = 10


def bound_and_exact(audio, sr, rms):
    """(float64 result of the contract from the f32 levelled signal, the per-sample bound) for one prompt."""
    v = audio.mean(dim=0) if audio.shape[0] > 1 else audio[0]
    if rms < TARGET_RMS:
        v = v * TARGET_RMS / rms
    k, orig, new, width = resample_kernel(sr, TARGET)
    bank = k[:, 0].to(torch.float32).double()
    K = bank.shape[1]
    n = v.shape[0]
    L = -(-new * n // orig)
    frames = -(-L // new)
    x = torch.zeros(width + frames * orig + K, dtype=torch.float64)
    x[width:width + n] = v.double()
    win = x.unfold(0, K, orig)[:frames]                       # [frames, K]
    y = win @ bank.t()
    mag = win.abs() @ bank.abs().t()
    return y.reshape(-1)[:L], ((K + 1) * 2.0 ** -24 * mag).reshape(-1)[:L]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if args.reps < 1 or args.warmup < 1:
        ap.error("--reps and --warmup must be >= 1")
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool only measures on the device")
    ms = P.mel.MelSpec()
    for name, (B, ch, sr) in SHAPES.items():
        audios = [torch.randn(ch, SECONDS * sr, generator=torch.Generator().manual_seed(1000 * b + ch)) * 0.05 for b in range(B)]
        rates = [sr] * B

        def host():
            norm = [I.normalise_prompt(a, sr, TARGET_RMS) for a in audios]
            down = torch.cat([a[0] for a, _ in norm]).to(DEV)                          # forward_ragged's one copy
            return list(down.split([a.shape[-1] for a, _ in norm])), [r for _, r in norm]

        def device():
            return ms.prepare_ragged(audios, rates, TARGET_RMS, device=DEV)

        variants = {"host": host, "device": device}
        for _ in range(args.warmup):
            for fn in variants.values():
                fn()
        torch.cuda.synchronize()
        hw, hr = host()
        dw, dr = device()
        dr = dr.cpu()
        worst = 0.0
        for b in sorted({0, B - 1}):
            exact, bound = bound_and_exact(audios[b], sr, torch.tensor(hr[b]))
            for got in (hw[b], dw[b]):
                worst = max(worst, float(((got.cpu().double() - exact).abs() / bound.clamp_min(1e-300)).max()))
        rms_rel = max(abs(float(dr[b]) - hr[b]) / hr[b] for b in range(B))
        dev_ms = {k: [] for k in variants}
        wall_ms = {k: [] for k in variants}
        for _ in range(args.reps):
            for k, fn in variants.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                a.record()
                fn()
                b.record()
                b.synchronize()
                wall_ms[k].append((time.perf_counter() - t0) * 1e3)
                dev_ms[k].append(a.elapsed_time(b))
        rec = {"shape": name, "items": B, "channels": ch, "rate": sr, "seconds_each": SECONDS, "reps": args.reps,
               "host_wall_ms_median": round(statistics.median(wall_ms["host"]), 3),
               "device_wall_ms_median": round(statistics.median(wall_ms["device"]), 3),
               "host_wall_ms_min_max": [round(min(wall_ms["host"]), 3), round(max(wall_ms["host"]), 3)],
               "device_wall_ms_min_max": [round(min(wall_ms["device"]), 3), round(max(wall_ms["device"]), 3)],
               "host_stream_ms_median": round(statistics.median(dev_ms["host"]), 3),
               "device_stream_ms_median": round(statistics.median(dev_ms["device"]), 3),
               "worst_error_over_bound": round(worst, 4), "rms_max_rel_diff": float(f"{rms_rel:.3g}"),
               "device_launches": 3, "device_h2d_copies": 2}
        rec["host_over_device_wall"] = round(rec["host_wall_ms_median"] / rec["device_wall_ms_median"], 2)
        print(json.dumps(rec), flush=True)
        assert worst <= 1.0, "a result lies outside the forward error bound"
        assert rms_rel <= 1e-5, "the device rms differs from the host's"          # (the host sums 10 s of squares in f32)


if __name__ == "__main__":
    main()
