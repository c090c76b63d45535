"""What isolated rows cost and buy (DiT.set_isolated_rows; open_pool(isolate=True)), each against the same leg without them:
(a) tools/pool_slice_time.py's pool of 16 clients at four settings, slice_steps=16, length buckets of 64, with and without isolate:
    audio seconds per wall second and the worst client's first packet;
(b) a live-like pool: every round each client submits a text of another length, drawn from a seeded generator, so a tick rarely
    repeats an exact (N, text length, distinct times); graph_stats() of both engines after the rounds;
(c) one mixed tick as a sample_items call: one 300-frame row beside fifteen 1,000-frame rows.

    python tools/pool_isolate_time.py [--runs 30] [--clients 16] [--bucket 64] [--out FILE.json]

F5-TTS Base with synthetic weights, Vocos 24 kHz, cfg 2 / 1.5, sway -1, NFE 16 / 32.  Two models of the same weights, one with the
switch: the legs alternate inside every round, two warm-up rounds, the median of --runs with min - max; a device synchronise, a host
clock around the leg and a device synchronise.  The non-isolated leg is the yardstick: it is what the pool did before."""
import argparse
import json
import os
import random
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import f5_tts_amd as P  # noqa: E402
from f5_tts_amd import infer as I  # noqa: E402
from sample_items_time import DEV, MIX, REF_TEXT, TEXT, run_pool, save, spread, timed  # noqa: E402

SENTENCES = TEXT.split(". ")


def pools(models, voc, K, batch_frames, slice_steps):
    """One pool per model ("isolate", "rectangular"), each with K clients at tools/sample_items_time.py's four settings."""
    audio = torch.randn(1, 240000, generator=torch.Generator().manual_seed(5)) * 0.05
    base = dict(nfe_step=16, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=0)
    own = [dict(nfe_step=(16, 32)[i % 2], cfg_strength=(2.0, 1.5)[(i // 2) % 2]) for i in range(K)]
    mix = [MIX[i % len(MIX)] for i in range(K)]
    out = {}
    for name, model in models.items():
        bank = I.prepare_voices(model, {"main": dict(ref_audio=(audio, 24000), ref_text=REF_TEXT)})
        pool = I.open_pool(model, voc, bank, batch_frames=batch_frames, slice_steps=slice_steps, isolate=name == "isolate", **base)
        out[name] = (pool, [pool.connect("main", out_rate=r, sample_format=f, **kw) for (r, f), kw in zip(mix, own)])
    return out, mix


def run_live(pool, clients, texts):
    """run_pool with a text per client."""
    t0 = time.perf_counter()
    reqs = []
    for c, text in zip(clients, texts):
        c.reset()
        reqs.append(c.submit(text))
    firsts, counts = {r.id: None for r in reqs}, {r.id: 0 for r in reqs}
    for r, packet, _rate in pool.run():
        if firsts[r.id] is None:
            firsts[r.id] = (time.perf_counter() - t0) * 1e3
        counts[r.id] += len(packet)
    return [firsts[r.id] for r in reqs], [counts[r.id] for r in reqs]


def pool_legs(models, voc, K, batch_frames, runs, live):
    legs, mix = pools(models, voc, K, batch_frames, 16)
    rng = random.Random(7)
    times = {name: [] for name in legs}
    for name in legs:
        models[name].transformer.graph_stats(reset=True)
    for r in range(runs + 2):
        texts = [". ".join(SENTENCES[:rng.randint(3, len(SENTENCES))]) + "." for _ in range(K)] if live else None
        for name, (pool, clients) in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            firsts, counts = run_live(pool, clients, texts) if live else run_pool(pool, clients)
            total = time.perf_counter() - t0
            torch.cuda.synchronize()
            audio_s = sum(n / rate for n, (rate, _) in zip(counts, mix))
            if r >= 2:
                times[name].append((audio_s / total, max(firsts), total * 1e3))
    out = {"clients": K, "settings": 4, "live_lengths": bool(live)}
    for name, ts in times.items():
        out[name] = {"audio_s_per_wall_s": spread([t[0] for t in ts]), "first_packet_ms_worst_client": spread([t[1] for t in ts]),
                     "total_ms": spread([t[2] for t in ts]), "stats": legs[name][0].stats(),
                     "graph_stats": models[name].transformer.graph_stats()}
    return out


def mixed_tick(models, runs, rows=16, short=300, long=1000, prompt=256, nt=120):
    g = torch.Generator().manual_seed(3)
    cond = torch.randn(rows, prompt, 100, generator=g).to(DEV)
    text = torch.randint(0, 2000, (rows, nt), generator=g)
    dur, lens = torch.tensor([short] + [long] * (rows - 1)), torch.full((rows,), prompt)
    kw = dict(steps=[16] * rows, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=0)
    times = {name: [] for name in models}
    for r in range(runs + 2):
        for name, model in models.items():
            t = timed(lambda: model.sample_items(cond, text, dur, lens=lens, **kw))
            if r >= 2:
                times[name].append(t)
    return {"rows": rows, "frames": [short] + [long] * (rows - 1), **{name: spread(ts) for name, ts in times.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--clients", type=int, default=16)
    ap.add_argument("--bucket", type=int, default=64)
    ap.add_argument("--precision", default="f16p")
    ap.add_argument("--batch-frames", type=int, default=40000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pool_isolate_time.py measures on the GPU: none is visible")
    models = {}
    for name in ("isolate", "rectangular"):
        tr = P.DiT(**P.config.F5TTS_BASE, text_num_embeds=P.config.VOCAB_SIZE + 1, mel_dim=100, precision=args.precision).init_synthetic(seed=0)
        tr.set_length_buckets(args.bucket)
        models[name] = P.CFM(transformer=tr, mel_spec_module=P.mel.MelSpec()).to(DEV)
    voc = P.Vocos(P.config.VOCOS_24K).init_synthetic(seed=1).to(DEV)
    rec = {"tool": "pool_isolate_time", "precision": args.precision, "bucket": args.bucket, "runs": args.runs, "slice_steps": 16,
           "batch_frames": args.batch_frames, "clock": "host perf_counter between device synchronises"}
    for key, live in (("pool", False), ("pool_live_lengths", True)):
        rec[key] = pool_legs(models, voc, args.clients, args.batch_frames, args.runs, live)
        print(json.dumps({key: rec[key]}), flush=True)
        if args.out:
            save(rec, args.out)
    models["isolate"].transformer.set_isolated_rows(True)        # (the pool turned it on already; said again for the sampler leg)
    rec["mixed_tick_ms"] = mixed_tick(models, args.runs)
    print(json.dumps(rec))
    if args.out:
        save(rec, args.out)


if __name__ == "__main__":
    main()
