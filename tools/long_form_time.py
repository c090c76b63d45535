"""What one long text costs through infer_batch_process, chunk by chunk against one ragged batch (F5-TTS Base f16p, Vocos
24 kHz, synthetic weights; NFE 16, cfg 2.0, sway -1: bench.py's C2 settings).

  sequential  infer_batch_process(..., batched=False): per chunk a prompt mel, a B = 1 sample(), a Vocos decode and a copy to
              the host, then the numpy cross-fade
  batched     infer_batch_process(..., batched=True): one prompt mel, one ragged sample(), one decode_ragged, one
              f5_wave_crossfade, one copy to the host

for the same prompt (256 frames = 2.73 s, 40 bytes of text) and K = 2, 4, 8 chunks of 96 .. 120 bytes, i.e. totals of 855 .. 1005
frames per chunk (C2 runs 1024).  Both variants end with the finished waveform on the host, so a repetition is timed
between two events on the stream around the whole call; the variants alternate inside one process, --warmup untimed
repetitions of every K come first (code objects, arena growth, graph captures), and the medians of --reps repetitions are
printed as ONE JSON line.

    python tools/long_form_time.py [--reps 5] [--warmup 2] [--variants sequential,batched]
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
import f5_tts_amd as P  # noqa: E402
from f5_tts_amd import infer as I  # noqa: E402

DEV = "cuda:0"
REF_FRAMES = 256
REF_TEXT = ("the quick brown fox jumps over the dog " * 2)[:39] + "."          # 40 bytes; + the trailing space rule: 41
GEN_BYTES = [120, 104, 112, 96, 118, 100, 108, 114]                              # per chunk; the first K are used


def chunk(n: int, k: int) -> str:
    words = "lorem ipsum dolor sit amet consectetur adipiscing elit sed do eiusmod tempor incididunt ut labore et dolore magna aliqua "
    return (words[k:] + words * 2)[:n - 1] + "."


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--variants", default="sequential,batched")
    ap.add_argument("--chunks", default="2,4,8")
    args = ap.parse_args()
    variants = args.variants.split(",")
    if args.reps < 1 or args.warmup < 1 or not set(variants) <= {"sequential", "batched"}:
        ap.error("--reps and --warmup must be >= 1; --variants: sequential, batched")
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool only measures on the device")
    P.utils.configure_host_threads(1)
    tr = P.DiT(**P.config.F5TTS_BASE, text_num_embeds=257, mel_dim=100, precision="f16p").init_synthetic(seed=0)
    model = P.CFM(transformer=tr).to(DEV)
    voc = P.Vocos(P.config.VOCOS_24K).init_synthetic(seed=1).to(DEV)
    audio = torch.randn(1, REF_FRAMES * 256, generator=torch.Generator().manual_seed(2)) * 0.05
    kw = dict(nfe_step=16, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=0)
    ks = [int(k) for k in args.chunks.split(",")]

    def run(variant, texts):
        extra = {"batched": True} if variant == "batched" else {}
        return next(I.infer_batch_process((audio, 24000), REF_TEXT, texts, model, voc, **kw, **extra))

    rec = {"tool": "long_form_time", "model": "F5-TTS Base f16p, synthetic weights", "vocoder": "Vocos 24 kHz",
           "prompt_frames": REF_FRAMES, "nfe": 16, "reps": args.reps, "warmup": args.warmup, "results": []}
    cases = {k: [chunk(n, i) for i, n in enumerate(GEN_BYTES[:k])] for k in ks}
    for texts in cases.values():
        for _ in range(args.warmup):
            for v in variants:
                run(v, texts)
    torch.cuda.synchronize()
    for k, texts in cases.items():
        frames = [I.prompt_numerics(audio, 24000, REF_TEXT, t)[4] for t in texts]
        ms = {v: [] for v in variants}
        wall = {v: [] for v in variants}
        waves = {}
        for _ in range(args.reps):
            for v in variants:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                a.record()
                waves[v] = run(v, texts)[0]
                b.record()
                b.synchronize()
                wall[v].append((time.perf_counter() - t0) * 1e3)
                ms[v].append(a.elapsed_time(b))
        r = {"chunks": k, "frames_per_chunk": frames, "audio_s": round(len(next(iter(waves.values()))) / 24000, 2)}
        for v in variants:
            r[f"{v}_ms_median"] = round(statistics.median(ms[v]), 2)
            r[f"{v}_ms_min_max"] = [round(min(ms[v]), 2), round(max(ms[v]), 2)]
            r[f"{v}_wall_ms_median"] = round(statistics.median(wall[v]), 2)
        if len(variants) == 2:
            r["sequential_over_batched"] = round(r["sequential_ms_median"] / r["batched_ms_median"], 3)
            # attn_mask_enabled=False: a shorter chunk attends over the batch's padding, so the two differ (infer.synthesize_long)
            seq, bat = waves["sequential"].astype(np.float32), waves["batched"]
            r["wave_linf_between_variants"] = float(np.abs(seq - bat).max()) if seq.shape == bat.shape else None
            r["wave_peak"] = float(np.abs(seq).max())
        rec["results"].append(r)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
