"""What the prompt mels of a batch of speakers cost item by item against one ragged pass (vocos front-end: n_fft 1024, hop 256).

  loop    mels = [ms(w[None]) for w in wavs]; then the zero-pad and stack of padded_mel_batch          (the reference's
          eval/utils_eval.py:109-148, 17-25): B calls of f5_mel_forward_ex (1 + 3 launches each) and B + 1 torch ops
  ragged  ms.forward_ragged(wavs): one call of f5_mel_forward_ragged (5 launches and one table copy)

on two batches of prompts that are already on the device (random samples; the cost does not depend on them):

  long   32 prompts of 3 - 10 s   (72,000 .. 240,000 samples, seed 1234)
  short  64 prompts of 1 - 3 s    (24,000 .. 72,000 samples, seed 1234)

Both variants run in this process, alternating, each repetition between two events on the stream; the medians of --reps
repetitions after --warmup untimed ones are printed with the host time per repetition (time to enqueue), the launch counts
and a bit-comparison of the two padded batches.

    python tools/mel_ragged_time.py [--reps 30] [--warmup 5]
    rocprofv3 --kernel-trace --stats -- python tools/mel_ragged_time.py --reps 3 --warmup 1     # per-kernel times, own run
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

DEV = "cuda:0"
SR = 24000


def batches():
    gl = torch.Generator().manual_seed(1234)
    long = [int(x) for x in torch.randint(3 * SR, 10 * SR + 1, (32,), generator=gl)]
    gs = torch.Generator().manual_seed(1234)
    short = [int(x) for x in torch.randint(1 * SR, 3 * SR + 1, (64,), generator=gs)]
    return {"long": long, "short": short}


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
    for name, nws in batches().items():
        B = len(nws)
        wavs = [(torch.randn(nw, generator=torch.Generator().manual_seed(nw)) * 0.1).to(DEV) for nw in nws]
        frames = [nw // ms.hop_length + 1 for nw in nws]
        T = max(frames)

        def loop():
            mels = [ms(w[None]) for w in wavs]                                           # [1, 100, T_b] each
            return torch.stack([torch.nn.functional.pad(m[0], (0, T - m.shape[-1]), value=0) for m in mels])

        def ragged():
            return ms.forward_ragged(wavs)[0]

        variants = {"loop": loop, "ragged": ragged}
        for _ in range(args.warmup):        # every shape of the timed window, workspace grown to its largest
            for fn in variants.values():
                fn()
        torch.cuda.synchronize()
        same = torch.equal(loop().view(torch.int32), ragged().view(torch.int32))
        dev_ms = {k: [] for k in variants}
        host_ms = {k: [] for k in variants}
        for _ in range(args.reps):
            for k, fn in variants.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                a.record()
                fn()
                b.record()
                host_ms[k].append((time.perf_counter() - t0) * 1e3)
                b.synchronize()
                dev_ms[k].append(a.elapsed_time(b))
        rec = {
            "batch": name, "items": B, "frames": sum(frames), "frames_min_max": [min(frames), max(frames)],
            "audio_s": round(sum(nws) / SR, 2), "reps": args.reps, "bit_identical": same,
            "loop_ms_median": round(statistics.median(dev_ms["loop"]), 3), "ragged_ms_median": round(statistics.median(dev_ms["ragged"]), 3),
            "loop_ms_min_max": [round(min(dev_ms["loop"]), 3), round(max(dev_ms["loop"]), 3)],
            "ragged_ms_min_max": [round(min(dev_ms["ragged"]), 3), round(max(dev_ms["ragged"]), 3)],
            "loop_host_ms_median": round(statistics.median(host_ms["loop"]), 3),
            "ragged_host_ms_median": round(statistics.median(host_ms["ragged"]), 3),
            "loop_launches": 4 * B, "loop_torch_ops": B + 1, "ragged_launches": 5, "ragged_h2d_copies": 1,
        }
        rec["loop_over_ragged"] = round(rec["loop_ms_median"] / rec["ragged_ms_median"], 3)
        print(json.dumps(rec), flush=True)
        assert same, "the two variants disagree"


if __name__ == "__main__":
    main()
