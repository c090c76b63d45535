"""What per-item sampler settings cost: (a) a uniform CFM.sample_items against CFM.sample at the same shape -- the price of the
gather launch per evaluation and of the general update kernels --, and a batch of mixed step counts against the two uniform calls
it replaces; (b) a stream pool whose K clients differ in their settings against the only alternative without sample_items: one
pool per distinct setting, run one after another.

    python tools/sample_items_time.py [--runs 30] [--pool-runs 8] [--batch 16] [--clients 16] [--precision f16p] [--out FILE.json]
    python tools/sample_items_time.py --trace-leg {sample|items}      # three calls of one leg, for a kernel trace of its own

F5-TTS Base with synthetic weights, Vocos 24 kHz.  (a): B = --batch items of a 256-frame prompt and 1,000 frames in all, NFE 16 and
32, cfg 2, sway -1, graphs on (the timed calls replay); a device synchronise, a host clock around the call and a device
synchronise; the legs alternate inside every round, two warm-up rounds, the median of --runs with min - max.  (b): the prompt and
the request of tools/pool_time.py, client i at NFE (16, 32)[i % 2] and cfg (2.0, 1.5)[(i // 2) % 2] -- four settings --, every
client submits at the start of a round; audio seconds per wall second and the worst client's first packet, median of --pool-runs
with min - max.  The alternative's first packet of a client counts from the start of the round: its pool waits for the pools in
front of it."""
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
REF_TEXT = ("This prompt has exactly one hundred bytes of text. " * 2)[:99] + "."
TEXT = " ".join("Sentence number %02d has thirtysix b." % i for i in range(16))
MIX = [(24000, "f32"), (16000, "s16"), (44100, "s16"), (48000, "f32"), (8000, "s16"), (22050, "f32")]


def spread(values):
    return {"median": round(statistics.median(values), 3), "min_max": [round(min(values), 3), round(max(values), 3)]}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def batch_inputs(B, prompt=256, total=1000, nt=120):
    g = torch.Generator().manual_seed(3)
    cond = torch.randn(B, prompt, 100, generator=g).to(DEV)
    text = torch.randint(0, 2000, (B, nt), generator=g)
    return cond, text, torch.full((B,), total), torch.full((B,), prompt)


def sampler_legs(model, B):
    cond, text, dur, lens = batch_inputs(B)
    kw = dict(cfg_strength=2.0, sway_sampling_coef=-1.0, seed=0)
    half = B // 2
    mixed_steps = [16] * half + [32] * (B - half)

    def sub(t, a, b):
        return t[a:b].contiguous()

    return {
        "sample_nfe16": lambda: model.sample(cond, text, dur, lens=lens, steps=16, **kw),
        "items_uniform_nfe16": lambda: model.sample_items(cond, text, dur, lens=lens, steps=16, **kw),
        "sample_nfe32": lambda: model.sample(cond, text, dur, lens=lens, steps=32, **kw),
        "items_uniform_nfe32": lambda: model.sample_items(cond, text, dur, lens=lens, steps=32, **kw),
        "items_mixed_16_32": lambda: model.sample_items(cond, text, dur, lens=lens, steps=mixed_steps, **kw),
        "two_samples_16_32": lambda: (model.sample(sub(cond, 0, half), sub(text, 0, half), dur[:half], lens=lens[:half], steps=16, **kw),
                                      model.sample(sub(cond, half, B), sub(text, half, B), dur[half:], lens=lens[half:], steps=32, **kw)),
    }


def run_pool(pool, clients, t0=None, kw_of=None):
    t0 = time.perf_counter() if t0 is None else t0
    reqs = []
    for c in clients:
        c.reset()
        reqs.append(c.submit(TEXT))
        if kw_of is not None:
            kw_of[reqs[-1].id] = tuple(sorted(c.sample_kw.items(), key=str))
    firsts, counts = {r.id: None for r in reqs}, {r.id: 0 for r in reqs}
    for r, packet, _rate in pool.run():
        if firsts[r.id] is None:
            firsts[r.id] = (time.perf_counter() - t0) * 1e3
        counts[r.id] += len(packet)
    return [firsts[r.id] for r in reqs], [counts[r.id] for r in reqs]


def pool_legs(model, voc, K, batch_frames, runs):
    audio = torch.randn(1, 240000, generator=torch.Generator().manual_seed(5)) * 0.05
    bank = I.prepare_voices(model, {"main": dict(ref_audio=(audio, 24000), ref_text=REF_TEXT)})
    base = dict(nfe_step=16, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=0)
    own = [dict(nfe_step=(16, 32)[i % 2], cfg_strength=(2.0, 1.5)[(i // 2) % 2]) for i in range(K)]
    mix = [MIX[i % len(MIX)] for i in range(K)]
    one = I.open_pool(model, voc, bank, batch_frames=batch_frames, **base)
    one_clients = [one.connect("main", out_rate=r, sample_format=f, **kw) for (r, f), kw in zip(mix, own)]
    settings = sorted({tuple(sorted(kw.items())) for kw in own})
    split = []
    for s in settings:
        pool = I.open_pool(model, voc, bank, batch_frames=batch_frames, **dict(base, **dict(s)))
        members = [i for i, kw in enumerate(own) if tuple(sorted(kw.items())) == s]
        split.append((pool, [pool.connect("main", out_rate=mix[i][0], sample_format=mix[i][1]) for i in members], members))

    kw_of = {}   # request id -> the settings it ran with (to count the ticks that mixed settings)

    def mixed_pool():
        return run_pool(one, one_clients, kw_of=kw_of)

    def pool_per_setting():
        t0 = time.perf_counter()
        firsts, counts = [None] * K, [0] * K
        for pool, clients, members in split:
            f, c = run_pool(pool, clients, t0)
            for i, fi, ci in zip(members, f, c):
                firsts[i], counts[i] = fi, ci
        return firsts, counts

    times = {"mixed_pool": [], "pool_per_setting": []}
    for r in range(runs + 2):
        for name, leg in (("mixed_pool", mixed_pool), ("pool_per_setting", pool_per_setting)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            firsts, counts = leg()
            total = time.perf_counter() - t0
            torch.cuda.synchronize()
            audio_s = sum(n / rate for n, (rate, _) in zip(counts, mix))
            if r >= 2:
                times[name].append((audio_s / total, max(firsts), total * 1e3))
    out = {"clients": K, "settings": len(settings), "audio_seconds_per_round": round(audio_s, 2),
           "mixed_pool_stats": one.stats(), "mixed_pool_ticks_of_mixed_settings": sum(1 for tick in one.log if len({kw_of[rid] for rid, _ in tick}) > 1)}
    for name, ts in times.items():
        out[name] = {"audio_s_per_wall_s": spread([t[0] for t in ts]), "first_packet_ms_worst_client": spread([t[1] for t in ts]),
                     "total_ms": spread([t[2] for t in ts])}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--pool-runs", type=int, default=8)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--clients", type=int, default=16)
    ap.add_argument("--precision", default="f16p")
    ap.add_argument("--batch-frames", type=int, default=40000)
    ap.add_argument("--trace-leg", choices=["sample", "items"], default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sample_items_time.py measures on the GPU: none is visible")
    tr = P.DiT(**P.config.F5TTS_BASE, text_num_embeds=P.config.VOCAB_SIZE + 1, mel_dim=100, precision=args.precision).init_synthetic(seed=0)
    model = P.CFM(transformer=tr, mel_spec_module=P.mel.MelSpec()).to(DEV)
    legs = sampler_legs(model, args.batch)
    if args.trace_leg:   # a kernel trace of its own: eager, capture, replay of one leg and nothing else
        leg = legs["sample_nfe16" if args.trace_leg == "sample" else "items_uniform_nfe16"]
        for _ in range(3):
            leg()
        torch.cuda.synchronize()
        return
    rec = {"tool": "sample_items_time", "precision": args.precision, "batch": args.batch, "frames": 1000, "prompt_frames": 256,
           "runs": args.runs, "clock": "host perf_counter between device synchronises", "sampler_ms": {}}
    times = {name: [] for name in legs}
    for r in range(args.runs + 2):
        for name, leg in legs.items():
            t = timed(leg)
            if r >= 2:
                times[name].append(t)
    rec["sampler_ms"] = {name: spread(ts) for name, ts in times.items()}
    rec["graph_stats_after_sampler_legs"] = tr.graph_stats()
    print(json.dumps(rec["sampler_ms"]), flush=True)
    if args.out:
        save(rec, args.out)
    if args.clients > 0:
        voc = P.Vocos(P.config.VOCOS_24K).init_synthetic(seed=1).to(DEV)
        rec["pool"] = pool_legs(model, voc, args.clients, args.batch_frames, args.pool_runs)
    print(json.dumps(rec))
    if args.out:
        save(rec, args.out)


def save(rec, path):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
