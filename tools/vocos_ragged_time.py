"""What decoding a ragged batch item by item costs against one ragged pass (Vocos 24 kHz, synthetic weights).

  loop    [voc.decode(out[i:i+1, refs[i]:durs[i], :].permute(0, 2, 1)) for i in range(B)]     (bench.py's ragged workload,
          the reference's eval_infer_batch.py:202-212): B calls of f5_vocos_decode_strided
  ragged  voc.decode_ragged(out.permute(0, 2, 1), ends=durs, starts=refs): one call of f5_vocos_decode_ragged

on two batches of sample()-shaped mels [B, N, 100] (random values; the decode's cost does not depend on them):

  c3     bench.py's C3 lengths: 32 items, N_i = 1024 then U{384..1024} (seed 1234), prompt N_i // 4
  short  64 short items: N_i ~ U{48..160} (seed 1234), prompt N_i // 4  -- 37 .. 118 generated frames (0.4 .. 1.3 s) each

Both variants run in this process, alternating, each repetition between two events on the stream; the medians of --reps
repetitions after --warmup untimed ones are printed with the host time per repetition (time to enqueue), the launch
counts (kernels per decode = 8 + 3 x layers, from csrc/vocos.hip; the ragged call adds one host-to-device copy of its
tables) and a bit-comparison of the two results.

    python tools/vocos_ragged_time.py [--reps 30] [--warmup 5]
    rocprofv3 --kernel-trace --stats -- python tools/vocos_ragged_time.py --reps 3 --warmup 1     # per-kernel times, own run
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


def batches():
    gl = torch.Generator().manual_seed(1234)
    c3 = [1024] + [int(x) for x in torch.randint(384, 1025, (31,), generator=gl)]      # bench.py make_inputs("c3"), rank 0
    gs = torch.Generator().manual_seed(1234)
    short = [int(x) for x in torch.randint(48, 161, (64,), generator=gs)]
    return {"c3": c3, "short": short}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if args.reps < 1 or args.warmup < 1:
        ap.error("--reps and --warmup must be >= 1")
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool only measures on the device")
    cfg = P.config.VOCOS_24K
    voc = P.Vocos(cfg).init_synthetic(seed=1).to(DEV)
    per_decode = 8 + 3 * cfg["num_layers"]
    for name, durs in batches().items():
        B, refs = len(durs), [d // 4 for d in durs]
        out = torch.randn(B, max(durs), 100, generator=torch.Generator().manual_seed(2)).to(DEV)
        frames = sum(d - r for d, r in zip(durs, refs))

        def loop():
            return [voc.decode(out[i:i + 1, refs[i]:durs[i], :].permute(0, 2, 1)) for i in range(B)]

        def ragged():
            return voc.decode_ragged(out.permute(0, 2, 1), ends=durs, starts=refs)

        variants = {"loop": loop, "ragged": ragged}
        for _ in range(args.warmup):        # every shape of the timed window, workspace grown to its largest
            for fn in variants.values():
                fn()
        torch.cuda.synchronize()
        wavs = loop()
        wav, wav_lens = ragged()
        same = all(torch.equal(wav[i, :wav_lens[i]].view(torch.int32), wavs[i][0].view(torch.int32)) for i in range(B))
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
            "batch": name, "items": B, "generated_frames": frames, "frames_min_max": [min(d - r for d, r in zip(durs, refs)), max(d - r for d, r in zip(durs, refs))],
            "audio_s": round(frames * cfg["hop_length"] / 24000, 2), "reps": args.reps, "bit_identical": same,
            "loop_ms_median": round(statistics.median(dev_ms["loop"]), 3), "ragged_ms_median": round(statistics.median(dev_ms["ragged"]), 3),
            "loop_ms_min_max": [round(min(dev_ms["loop"]), 3), round(max(dev_ms["loop"]), 3)],
            "ragged_ms_min_max": [round(min(dev_ms["ragged"]), 3), round(max(dev_ms["ragged"]), 3)],
            "loop_host_ms_median": round(statistics.median(host_ms["loop"]), 3),
            "ragged_host_ms_median": round(statistics.median(host_ms["ragged"]), 3),
            "loop_launches": B * per_decode, "ragged_launches": per_decode, "ragged_h2d_copies": 1,
        }
        rec["loop_over_ragged"] = round(rec["loop_ms_median"] / rec["ragged_ms_median"], 3)
        print(json.dumps(rec), flush=True)
        assert same, "the two variants disagree"


if __name__ == "__main__":
    main()
