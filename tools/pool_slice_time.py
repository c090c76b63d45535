"""What solving in slices costs and buys (CFM.sample_span; open_pool(slice_steps=...)):
(a) a batch of 8 items at NFE 16 and 8 at NFE 32 as two span calls of 16 steps -- the second over the 8 rows that are left -- against
    one sample_items over all 16 rows for 32 steps and against the two sample() calls the batch replaces;
(b) a uniform NFE 32 batch as 32 / k span calls for k in 4, 8, 16 against one sample_items: the difference divided by the slice
    count is what a slice costs (text encoder, time rows, staging, eager copies, one graph launch);
(c) tools/sample_items_time.py's pool of 16 clients and four settings with slice_steps=16 and with None: audio seconds per wall
    second and the worst client's first packet;
(d) a late client: 16 clients are in full ticks, one more "arrives" --arrival-ms after a tick was enqueued and is submitted when the
    step() that is running returns; its first packet counted from the arrival, with slice_steps=4 and with None.

    python tools/pool_slice_time.py [--runs 30] [--pool-runs 8] [--late-runs 5] [--arrival-ms 50] [--out FILE.json]

F5-TTS Base with synthetic weights, Vocos 24 kHz, B = 16 items of a 256-frame prompt and 1,000 frames in all, cfg 2, sway -1, graphs
on (the timed calls replay); a device synchronise, a host clock around the call and a device synchronise; the legs alternate inside
every round, two warm-up rounds, the median of --runs with min - max."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import f5_tts_amd as P  # noqa: E402
from f5_tts_amd import infer as I  # noqa: E402
from sample_items_time import DEV, MIX, REF_TEXT, TEXT, batch_inputs, run_pool, save, spread, timed  # noqa: E402


def chain(model, cond, text, dur, lens, steps, count, kw):
    """The solve of a batch as span calls of `count` steps; rows that have made their steps leave."""
    keep, made, prev = list(range(len(steps))), 0, None
    while keep:
        idx = torch.tensor(keep)
        res = model.sample_span(cond[idx.to(cond.device)], text[idx], dur[idx], lens=lens[idx], steps=[steps[i] for i in keep],
                                start=[made] * len(keep), count=count, prev=prev, **kw)
        made += count
        left = [b for b, d in enumerate(res.done) if not d]
        keep, prev = [keep[b] for b in left], (res.state, left)


def sampler_legs(model, B):
    cond, text, dur, lens = batch_inputs(B)
    kw = dict(cfg_strength=2.0, sway_sampling_coef=-1.0, seed=0)
    half = B // 2
    mixed = [16] * half + [32] * (B - half)

    def sub(t, a, b):
        return t[a:b].contiguous()

    legs = {
        "mixed_two_spans_of_16": lambda: chain(model, cond, text, dur, lens, mixed, 16, kw),
        "mixed_one_sample_items": lambda: model.sample_items(cond, text, dur, lens=lens, steps=mixed, **kw),
        "mixed_two_samples": lambda: (model.sample(sub(cond, 0, half), sub(text, 0, half), dur[:half], lens=lens[:half], steps=16, **kw),
                                      model.sample(sub(cond, half, B), sub(text, half, B), dur[half:], lens=lens[half:], steps=32, **kw)),
        "nfe32_one_sample_items": lambda: model.sample_items(cond, text, dur, lens=lens, steps=32, **kw),
    }
    for k in (4, 8, 16):
        legs[f"nfe32_spans_of_{k}"] = (lambda k: lambda: chain(model, cond, text, dur, lens, [32] * B, k, kw))(k)
    return legs


def pools(model, voc, K, batch_frames, slice_steps, four_settings):
    """One pool per entry of slice_steps, each with K clients: at tools/sample_items_time.py's four settings, or all at the pool's."""
    audio = torch.randn(1, 240000, generator=torch.Generator().manual_seed(5)) * 0.05
    bank = I.prepare_voices(model, {"main": dict(ref_audio=(audio, 24000), ref_text=REF_TEXT)})
    base = dict(nfe_step=16, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=0)
    own = [dict(nfe_step=(16, 32)[i % 2], cfg_strength=(2.0, 1.5)[(i // 2) % 2]) if four_settings else {} for i in range(K)]
    mix = [MIX[i % len(MIX)] for i in range(K)]
    out = {}
    for name, s in slice_steps.items():
        pool = I.open_pool(model, voc, bank, batch_frames=batch_frames, slice_steps=s, **base)
        out[name] = (pool, [pool.connect("main", out_rate=r, sample_format=f, **kw) for (r, f), kw in zip(mix, own)])
    return out, mix


def pool_legs(model, voc, K, batch_frames, runs):
    legs, mix = pools(model, voc, K, batch_frames, {"slice_steps_16": 16, "slice_steps_none": None}, True)
    times = {name: [] for name in legs}
    for r in range(runs + 2):
        for name, (pool, clients) in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            firsts, counts = run_pool(pool, clients)
            total = time.perf_counter() - t0
            torch.cuda.synchronize()
            audio_s = sum(n / rate for n, (rate, _) in zip(counts, mix))
            if r >= 2:
                times[name].append((audio_s / total, max(firsts), total * 1e3))
    out = {"clients": K, "settings": 4, "audio_seconds_per_round": round(audio_s, 2)}
    for name, ts in times.items():
        out[name] = {"audio_s_per_wall_s": spread([t[0] for t in ts]), "first_packet_ms_worst_client": spread([t[1] for t in ts]),
                     "total_ms": spread([t[2] for t in ts]), "stats": legs[name][0].stats()}
    return out


def late_client(model, voc, K, batch_frames, runs, arrival_ms):
    """K clients at NFE 16 submit; after two ticks' worth of steps the tick that is enqueued next is the one the late client arrives
    in, arrival_ms after its step() began.  It is submitted when that step() returns; its first packet is counted from the arrival."""
    legs, _ = pools(model, voc, K, batch_frames, {"slice_steps_4": 4, "slice_steps_none": None}, False)
    times = {name: [] for name in legs}
    for r in range(runs + 1):
        for name, (pool, clients) in legs.items():
            late = pool.connect("main")
            reqs = []
            for c in clients:
                c.reset()
                reqs.append(c.submit(TEXT))
            per_tick = 1 if pool.slice_steps is None else -(-16 // pool.slice_steps)
            for _ in range(3 * per_tick):                                # the first chunks' tick, then two full ticks
                pool.step()
            torch.cuda.synchronize()
            arrive = time.perf_counter() + arrival_ms * 1e-3
            req, first = None, None
            while first is None:
                if req is not None and pool.idle():
                    raise SystemExit("the late client's request ended without a packet")
                got = pool.step()
                if req is None and time.perf_counter() >= arrive:
                    req = late.submit("A short first sentence for the late client.")
                for rr, packets in got:
                    if req is not None and rr is req and packets:
                        first = (time.perf_counter() - arrive) * 1e3
            for rr in reqs:
                rr.cancel()
            for _ in pool.run():
                pass
            torch.cuda.synchronize()
            if r >= 1:
                times[name].append(first)
    return {"clients_in_full_ticks": K, "arrival_ms_after_the_tick_began": arrival_ms,
            **{name: {"first_packet_ms": spread(ts)} for name, ts in times.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--pool-runs", type=int, default=8)
    ap.add_argument("--late-runs", type=int, default=5)
    ap.add_argument("--arrival-ms", type=float, default=50.0)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--clients", type=int, default=16)
    ap.add_argument("--precision", default="f16p")
    ap.add_argument("--batch-frames", type=int, default=40000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pool_slice_time.py measures on the GPU: none is visible")
    tr = P.DiT(**P.config.F5TTS_BASE, text_num_embeds=P.config.VOCAB_SIZE + 1, mel_dim=100, precision=args.precision).init_synthetic(seed=0)
    model = P.CFM(transformer=tr, mel_spec_module=P.mel.MelSpec()).to(DEV)
    rec = {"tool": "pool_slice_time", "precision": args.precision, "batch": args.batch, "frames": 1000, "prompt_frames": 256,
           "runs": args.runs, "clock": "host perf_counter between device synchronises"}
    legs = sampler_legs(model, args.batch)
    times = {name: [] for name in legs}
    for r in range(args.runs + 2):
        for name, leg in legs.items():
            t = timed(leg)
            if r >= 2:
                times[name].append(t)
    rec["sampler_ms"] = {name: spread(ts) for name, ts in times.items()}
    whole = rec["sampler_ms"]["nfe32_one_sample_items"]["median"]
    rec["ms_per_slice"] = {k: round((rec["sampler_ms"][f"nfe32_spans_of_{k}"]["median"] - whole) / (32 // k), 3) for k in (4, 8, 16)}
    rec["graph_stats_after_sampler_legs"] = tr.graph_stats()
    print(json.dumps({"sampler_ms": rec["sampler_ms"], "ms_per_slice": rec["ms_per_slice"]}), flush=True)
    if args.out:
        save(rec, args.out)
    if args.clients > 0:
        voc = P.Vocos(P.config.VOCOS_24K).init_synthetic(seed=1).to(DEV)
        rec["pool"] = pool_legs(model, voc, args.clients, args.batch_frames, args.pool_runs)
        print(json.dumps({"pool": rec["pool"]}), flush=True)
        if args.out:
            save(rec, args.out)
        rec["late_client"] = late_client(model, voc, args.clients, args.batch_frames, args.late_runs, args.arrival_ms)
    print(json.dumps(rec))
    if args.out:
        save(rec, args.out)


if __name__ == "__main__":
    main()
