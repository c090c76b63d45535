"""What editing a batch of recordings costs item by item, against infer.speech_edit.

  loop    per recording: normalise_prompt, MelSpec.forward, the torch.cat chain for the conditioning and the mask (the reference
          script, infer/speech_edit.py:137-232), model.sample(edit_mask=...), vocoder.decode, the rescale
  driver  infer.speech_edit over all recordings: one ragged mel pass, one f5_edit_assemble, per group one sample() and one ragged
          decode (and with --splice one f5_wave_splice)

for 8 and 32 recordings of 3 ... 10 s at 24 kHz (random samples at amplitude 0.05, so every item is levelled) with two spans each,
on the Base-size DiT and the 24 kHz Vocos with synthetic weights.  Both variants run in this process, alternating, each repetition
between two events on the stream and inside a wall clock that ends in a device synchronise; the medians of --reps repetitions after
--warmup untimed ones are printed in milliseconds, one JSON line per batch.  With attn_mask_enabled=False (the shipped configs) the
driver's shorter items attend over the group's padding, so its mels are not the loop's; the line reports the largest difference.

    python tools/speech_edit_time.py [--reps 30] [--warmup 2] [--nfe 32] [--batches 8,32] [--batch-frames 16384] [--splice]
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

DEV = "cuda:0"
SR, HOP, TARGET_RMS = 24000, 256, 0.1
TEXT = "Some call me optimist, others call me realist."


def recordings(B):
    """B recordings of 3 ... 10 s, two spans each at 20-30 % and 60-75 % of the recording, the second one re-timed."""
    items = []
    for b in range(B):
        seconds = 3.0 + 7.0 * b / max(B - 1, 1)
        audio = torch.randn(1, int(seconds * SR), generator=torch.Generator().manual_seed(100 + b)) * 0.05
        parts = [(0.20 * seconds, 0.30 * seconds), (0.60 * seconds, 0.75 * seconds)]
        items.append((audio, SR, TEXT, parts, [0.10 * seconds, 0.20 * seconds]))
    return items


def cat_chain(original_mel, parts, fix):
    """speech_edit.py:157-195 on the device."""
    dev = original_mel.device
    mel_cond = torch.zeros(1, 0, original_mel.shape[2], device=dev)
    mask = torch.zeros(1, 0, dtype=torch.bool, device=dev)
    fix, offset = list(fix), 0
    for start, end in parts:
        dur = fix.pop(0)
        sf, ef, pf = round(start * SR / HOP), round(end * SR / HOP), round(dur * SR / HOP)
        mel_cond = torch.cat((mel_cond, original_mel[:, offset:sf], torch.zeros(1, pf, original_mel.shape[2], device=dev)), dim=1)
        mask = torch.cat((mask, torch.ones(1, sf - offset, dtype=torch.bool, device=dev), torch.zeros(1, pf, dtype=torch.bool, device=dev)), dim=-1)
        offset = ef
    mel_cond = torch.cat((mel_cond, original_mel[:, offset:]), dim=1)
    return mel_cond, torch.nn.functional.pad(mask, (0, mel_cond.shape[1] - mask.shape[-1]), value=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--nfe", type=int, default=32)
    ap.add_argument("--batches", default="8,32")
    ap.add_argument("--batch-frames", type=int, default=16384)   # the reference's frame budget per batch
    ap.add_argument("--splice", action="store_true")
    args = ap.parse_args()
    if args.reps < 1 or args.warmup < 1:
        ap.error("--reps and --warmup must be >= 1")
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool only measures on the device")
    tr = P.DiT(**P.config.F5TTS_V1_BASE, text_num_embeds=257, mel_dim=100).init_synthetic(seed=2)
    model = P.CFM(transformer=tr).to(DEV)
    voc = P.Vocos(P.config.VOCOS_24K).init_synthetic(seed=4).to(DEV)
    kw = dict(cfg_strength=2.0, sway_sampling_coef=-1.0, seed=3)
    for B in [int(b) for b in args.batches.split(",")]:
        items = recordings(B)

        def loop():
            out = []
            with torch.inference_mode():
                for audio, sr, text, parts, fix in items:
                    a, rms = I.normalise_prompt(audio, sr, TARGET_RMS)
                    orig = model.mel_spec(a.to(DEV)).permute(0, 2, 1)
                    cond, mask = cat_chain(orig, parts, fix)
                    mel, _ = model.sample(cond, [text], cond.shape[1], steps=args.nfe, edit_mask=mask, **kw)
                    wave = voc.decode(mel.to(torch.float32).permute(0, 2, 1))[0]
                    out.append((I.rescale_to_prompt(wave, rms, TARGET_RMS), mel[0]))
            return out

        def driver():
            return I.speech_edit(model, voc, items, nfe_step=args.nfe, batch_frames=args.batch_frames, splice=args.splice, **kw)

        variants = {"loop": loop, "driver": driver}
        for _ in range(args.warmup):
            for fn in variants.values():
                fn()
        torch.cuda.synchronize()
        want, (waves, _, mels) = loop(), driver()
        assert all(w.shape == x[0].shape and torch.isfinite(w).all() for w, x in zip(waves, want))
        mel_diff = max(float((m.permute(1, 0) - x[1]).abs().max()) for m, x in zip(mels, want))
        stream_ms = {k: [] for k in variants}
        wall_ms = {k: [] for k in variants}
        for _ in range(args.reps):
            for k, fn in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                wall_ms[k].append((time.perf_counter() - t0) * 1e3)
                stream_ms[k].append(e0.elapsed_time(e1))
        frames = [m.shape[1] for m in mels]
        groups = I.group_chunks(frames, args.batch_frames)
        rec = {"recordings": B, "seconds": [3, 10], "nfe": args.nfe, "reps": args.reps, "splice": args.splice,
               "batch_frames": args.batch_frames, "frames_min_max_sum": [min(frames), max(frames), sum(frames)],
               "groups": len(groups), "padded_frames": sum(len(r) * max(frames[k] for k in r) for r in groups),
               "mel_max_abs_diff_driver_vs_loop": float(f"{mel_diff:.3g}")}
        for k in variants:
            rec[f"{k}_ms_median"] = round(statistics.median(stream_ms[k]), 2)
            rec[f"{k}_ms_min_max"] = [round(min(stream_ms[k]), 2), round(max(stream_ms[k]), 2)]
            rec[f"{k}_wall_ms_median"] = round(statistics.median(wall_ms[k]), 2)
        rec["loop_over_driver"] = round(rec["loop_ms_median"] / rec["driver_ms_median"], 2)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
