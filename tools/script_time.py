"""What a multi-voice script costs, one infer_process per tagged stretch against one synthesize_script (F5-TTS Base f16p, Vocos
24 kHz, synthetic weights; NFE 16, cfg 2.0, sway -1: bench.py's C2 settings).

  per_stretch  what a caller can do without synthesize_script, and what the reference's infer_cli.py does: parse the script,
               then per stretch infer_process(batched=True, prompt_on_device=True) -- the prompt prepared again, its mel
               again, a sample() and a decode per stretch, a copy to the host -- and np.concatenate on the host
  script       synthesize_script with the voices as a dict: the prompts of all voices in one pass, the chunks of all stretches
               in ragged batches of --batch-frames, one f5_wave_join, one copy to the host
  bank         the same with a VoiceBank prepared once outside the timed region (prepare_voices)

for three voices (prompts of 4.2, 6.5 and 8.8 s at 24 kHz, 16 kHz stereo and 44.1 kHz) and a script of --stretches tagged
stretches of 40 .. 110 bytes, every eighth one of 267 bytes (two or three chunks, cross-faded).  Every variant ends with the finished waveform on the host, so a repetition is timed between two
events on the stream around the whole call; the variants alternate inside one process, --warmup untimed repetitions come first
(code objects, arena growth, graph captures), and the medians of --reps repetitions are printed as ONE JSON line.

    python tools/script_time.py [--reps 30] [--warmup 2] [--stretches 40] [--batch-frames 16384] [--variants per_stretch,script,bank]
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
VARIANTS = ("per_stretch", "script", "bank")
WORDS = "lorem ipsum dolor sit amet consectetur adipiscing elit sed do eiusmod tempor incididunt ut labore et dolore magna aliqua "


def sentence(n: int, k: int) -> str:
    return (WORDS[k % 40:] + WORDS * 2)[:n - 1].strip() + "."


def make_voices():
    g = torch.Generator().manual_seed(2)
    return {
        "main": dict(ref_audio=(torch.randn(1, int(4.2 * 24000), generator=g) * 0.05, 24000), ref_text=sentence(44, 0)),
        "town": dict(ref_audio=(torch.randn(2, int(6.5 * 16000), generator=g) * 0.2, 16000), ref_text=sentence(70, 7), speed=1.1),
        "crier": dict(ref_audio=(torch.randn(1, int(8.8 * 44100), generator=g) * 0.08, 44100), ref_text=sentence(95, 13)),
    }


def make_script(stretches: int) -> str:
    names = ["main", "town", "crier"]

    def text(k):                                              # every eighth stretch is four sentences: two chunks, a cross-fade
        return " ".join(sentence(66, k + i) for i in range(4)) if k % 8 == 5 else sentence(40 + (k * 37) % 71, k)

    return " ".join(f"[{names[(k * 7 // 3) % 3]}] {text(k)}" for k in range(stretches))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--stretches", type=int, default=40)
    ap.add_argument("--batch-frames", type=int, default=16384)
    ap.add_argument("--variants", default=",".join(VARIANTS))
    args = ap.parse_args()
    variants = args.variants.split(",")
    if args.reps < 1 or args.warmup < 1 or args.stretches < 1 or not set(variants) <= set(VARIANTS):
        ap.error("--reps, --warmup and --stretches must be >= 1; --variants: " + ", ".join(VARIANTS))
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool only measures on the device")
    P.utils.configure_host_threads(1)
    tr = P.DiT(**P.config.F5TTS_BASE, text_num_embeds=257, mel_dim=100, precision="f16p").init_synthetic(seed=0)
    model = P.CFM(transformer=tr).to(DEV)
    voc = P.Vocos(P.config.VOCOS_24K).init_synthetic(seed=1).to(DEV)
    voices, script = make_voices(), make_script(args.stretches)
    kw = dict(nfe_step=16, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=0)
    bank = I.prepare_voices(model, voices) if "bank" in variants else None

    def run(variant):
        if variant == "per_stretch":
            waves = []
            for voice, text in I.parse_script(script, voices):
                v = voices[voice]
                waves.append(I.infer_process(v["ref_audio"], v["ref_text"], text, model, voc, show_info=None, batched=True,
                                             prompt_on_device=True, batch_frames=args.batch_frames, speed=v.get("speed", 1.0), **kw)[0])
            return np.concatenate(waves)
        wave = I.synthesize_script(model, voc, bank if variant == "bank" else voices, script, batch_frames=args.batch_frames, **kw)[0]
        return wave.cpu().numpy()

    for _ in range(args.warmup):
        for v in variants:
            run(v)
    torch.cuda.synchronize()
    ms, wall, waves = {v: [] for v in variants}, {v: [] for v in variants}, {}
    for _ in range(args.reps):
        for v in variants:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record()
            waves[v] = run(v)
            b.record()
            b.synchronize()
            wall[v].append((time.perf_counter() - t0) * 1e3)
            ms[v].append(a.elapsed_time(b))
    plan = I.script_plan(I.parse_script(script, voices), I.prepare_voices(model, voices).prompts())
    rec = {"tool": "script_time", "model": "F5-TTS Base f16p, synthetic weights", "vocoder": "Vocos 24 kHz", "nfe": 16,
           "voices": len(voices), "stretches": args.stretches, "chunks": len(plan["items"]), "batch_frames": args.batch_frames,
           "frames_min_max": [min(it[3] for it in plan["items"]), max(it[3] for it in plan["items"])],
           "audio_s": round(len(next(iter(waves.values()))) / 24000, 2), "reps": args.reps, "warmup": args.warmup}
    for v in variants:
        rec[f"{v}_ms_median"] = round(statistics.median(ms[v]), 2)
        rec[f"{v}_ms_min_max"] = [round(min(ms[v]), 2), round(max(ms[v]), 2)]
        rec[f"{v}_wall_ms_median"] = round(statistics.median(wall[v]), 2)
    for v in variants:
        if v != "per_stretch" and "per_stretch" in variants:
            rec[f"per_stretch_over_{v}"] = round(rec["per_stretch_ms_median"] / rec[f"{v}_ms_median"], 3)
            # attn_mask_enabled=False: a shorter chunk attends over its batch's padding, so the two differ (infer.synthesize_script)
            same = waves[v].shape == waves["per_stretch"].shape
            rec[f"wave_linf_per_stretch_to_{v}"] = float(np.abs(waves[v] - waves["per_stretch"]).max()) if same else None
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
