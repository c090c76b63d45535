"""What decoding a ragged batch item by item costs against one ragged pass (BigVGAN v2 24 kHz, synthetic weights).

  loop    [voc(out[i:i+1, refs[i]:durs[i], :].permute(0, 2, 1)) for i in range(B)]: B calls of the unchanged f5_bigvgan_forward at B = 1
  ragged  voc.forward_ragged(out.permute(0, 2, 1), ends=durs, starts=refs): one call of f5_bigvgan_forward_ragged

on the two batches of tools/vocos_ragged_time.py, sample()-shaped mels [B, N, 100] (random values; the cost does not depend on them):

  c3     bench.py's C3 lengths: 32 items, N_i = 1024 then U{384..1024} (seed 1234), prompt N_i // 4
  short  64 short items: N_i ~ U{48..160} (seed 1234), prompt N_i // 4  -- 37 .. 118 generated frames (0.4 .. 1.3 s) each

Both precisions ("f32", "f16x3") and both variants run in this process, alternating, each repetition between two events on the
stream; the medians of --reps repetitions after --warmup untimed ones are printed with the host time per repetition (time to
enqueue), the launch counts (kernels per pass, counted as csrc/bigvgan.hip launches them: 2 for conv_pre, per stage 2 for the
transposed convolution, 4 per (conv, conv) pair of every resblock -- 6 where a pair's operand is materialised -- and 1 mean, then 2
for the last activation and conv_post; the ragged call adds one host-to-device copy of its tables), the packed row counts and a
bit-comparison of the two results.  --max-frames bounds the ragged call's workspace (BigVGAN.forward_ragged).

    python tools/bigvgan_ragged_time.py [--reps 30] [--warmup 5] [--max-frames N]
    rocprofv3 --kernel-trace --stats -- python tools/bigvgan_ragged_time.py --reps 3 --warmup 1     # per-kernel times, own run
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
from tools.vocos_ragged_time import batches  # noqa: E402

DEV = "cuda:0"


def launches_per_pass(cfg):
    """Kernel launches of one pass over one time axis, as csrc/bigvgan.hip issues them with its default switches."""
    n, ch = 2, cfg["upsample_initial_channel"]
    for _ in cfg["upsample_rates"]:
        ch //= 2
        materialised = ch % 32 != 0 and not (ch % 4 == 0 and ch < 64)      # neither implicit GEMM nor the narrow kernel
        n += 2 + len(cfg["resblock_kernel_sizes"]) * len(cfg["resblock_dilation_sizes"]) * (6 if materialised else 4) + 1
    return n + 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--max-frames", type=int, default=None)
    args = ap.parse_args()
    if args.reps < 1 or args.warmup < 1:
        ap.error("--reps and --warmup must be >= 1")
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool only measures on the device")
    cfg = P.config.BIGVGAN_V2_24K
    vocs = {prec: P.BigVGAN(cfg, precision=prec).init_synthetic(seed=1).to(DEV) for prec in ("f32", "f16x3")}
    per_pass = launches_per_pass(cfg)
    for name, durs in batches().items():
        B, refs = len(durs), [d // 4 for d in durs]
        out = torch.randn(B, max(durs), 100, generator=torch.Generator().manual_seed(2)).to(DEV)
        frames = [d - r for d, r in zip(durs, refs)]
        rs, gap = vocs["f32"].ragged_plan(frames)
        groups = vocs["f32"]._ragged_groups(frames, args.max_frames)

        def loop(voc):
            return [voc(out[i:i + 1, refs[i]:durs[i], :].permute(0, 2, 1)) for i in range(B)]

        def ragged(voc):
            return voc.forward_ragged(out.permute(0, 2, 1), ends=durs, starts=refs, max_frames=args.max_frames)

        variants = {(prec, k): (lambda fn=fn, voc=voc: fn(voc)) for prec, voc in vocs.items() for k, fn in (("loop", loop), ("ragged", ragged))}
        for _ in range(args.warmup):        # every shape of the timed window, workspace grown to its largest
            for fn in variants.values():
                fn()
        torch.cuda.synchronize()
        print(f"[{name}] warm-up done", file=sys.stderr, flush=True)
        same = {}
        for prec, voc in vocs.items():
            wavs = loop(voc)
            wav, wav_lens = ragged(voc)
            same[prec] = all(torch.equal(wav[i, :wav_lens[i]].view(torch.int32), wavs[i][0, 0].view(torch.int32)) for i in range(B))
        dev_ms = {k: [] for k in variants}
        host_ms = {k: [] for k in variants}
        for rep in range(args.reps):
            if rep % 10 == 0:
                print(f"[{name}] repetition {rep} of {args.reps}", file=sys.stderr, flush=True)
            for k, fn in variants.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                a.record()
                fn()
                b.record()
                host_ms[k].append((time.perf_counter() - t0) * 1e3)
                b.synchronize()
                dev_ms[k].append(a.elapsed_time(b))
        for prec in vocs:
            rec = {
                "batch": name, "precision": prec, "items": B, "generated_frames": sum(frames), "frames_min_max": [min(frames), max(frames)],
                "packed_frames": rs[-1], "gap_frames": gap, "last_stage_rows": rs[-1] * vocs[prec].total_up, "groups": len(groups),
                "audio_s": round(sum(frames) * 256 / 24000, 2), "reps": args.reps, "bit_identical": same[prec],
            }
            for k in ("loop", "ragged"):
                rec[k + "_ms_median"] = round(statistics.median(dev_ms[prec, k]), 3)
                rec[k + "_ms_min_max"] = [round(min(dev_ms[prec, k]), 3), round(max(dev_ms[prec, k]), 3)]
                rec[k + "_host_ms_median"] = round(statistics.median(host_ms[prec, k]), 3)
            rec.update(loop_launches=B * per_pass, ragged_launches=len(groups) * per_pass, ragged_h2d_copies=len(groups))
            rec["loop_over_ragged"] = round(rec["loop_ms_median"] / rec["ragged_ms_median"], 3)
            print(json.dumps(rec), flush=True)
        assert all(same.values()), "the two variants disagree"


if __name__ == "__main__":
    main()
