"""What K concurrent streaming clients cost: a stream pool (infer.open_pool) against K streaming sessions (infer.open_stream) run one
after another -- the sessions' code is what a server had before the pool --, and f5_wave_emit against the wave_join + wave_deliver
chain on one tick's tables, in one process.

    python tools/pool_time.py [--runs 30] [--clients 1,4,16] [--nfe 16] [--precision f16p] [--granule 64] [--batch-frames 40000] [--out FILE.json]

F5-TTS Base with synthetic weights, Vocos 24 kHz, length buckets on, the prompt and the request of tools/stream_time.py (a 10 s
prompt with a 100-byte text; 16 sentences of 36 bytes, which a first package cuts into 6 chunks).  Client i receives
(24 kHz f32, 16 kHz s16, 44.1 kHz s16, 48 kHz f32, 8 kHz s16, 22.05 kHz f32)[i % 6]; every client sends the request as a first package.
  sessions   K sessions with lookahead 1, each chunk its own B = 1 sample(), one client after the other: client i's first packet waits
             for the clients in front of it
  pool       one pool, K clients that submit at the start of the round; ticks of at most --batch-frames rows x longest row
The legs alternate inside every round.  Clocks: a host clock (time.perf_counter) from the start of a leg to the arrival of a packet
on the host -- the generators hand out host arrays whose copy has been waited for --, and to the end of the leg, which is followed
by a device synchronise outside the window.  The emit comparison is a host clock around the calls and a device synchronise: it
includes the launches and the table copies, which is the difference between the two routes.  Reports per K the audio seconds per
wall second of each leg and the first-packet latency over the clients (median and worst client), each as the median over --runs
rounds after two warm-up rounds with min - max.  (The two legs do not speak bit-equal audio: the pool's chunks share batches, and
with the shipped `attn_mask_enabled=False` a chunk in a batch sees the batch's padding; tests/test_stream_pool_gpu.py has the
bit-for-bit statements.)  With --out the record is rewritten after every K."""
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


def run_sessions(sessions):
    """(ms to each client's first packet, total ms, samples per client): the sessions one after another."""
    t0 = time.perf_counter()
    firsts, counts = [], []
    for s in sessions:
        s.reset()
        first, n = None, 0
        for packet, _rate in s.stream(TEXT):
            if first is None:
                first = (time.perf_counter() - t0) * 1e3
            n += len(packet)
        firsts.append(first)
        counts.append(n)
    return firsts, (time.perf_counter() - t0) * 1e3, counts


def run_pool(pool, clients):
    t0 = time.perf_counter()
    reqs = []
    for c in clients:
        c.reset()
        reqs.append(c.submit(TEXT))
    firsts, counts = {r.id: None for r in reqs}, {r.id: 0 for r in reqs}
    for r, packet, _rate in pool.run():
        if firsts[r.id] is None:
            firsts[r.id] = (time.perf_counter() - t0) * 1e3
        counts[r.id] += len(packet)
    return [firsts[r.id] for r in reqs], (time.perf_counter() - t0) * 1e3, [counts[r.id] for r in reqs]


def emit_against_chain(model, runs, streams_n=16):
    """One tick's tables: `streams_n` requests of three 2 s pieces each, a 3600-sample fade, growing, at the mixed rates."""
    g = torch.Generator().manual_seed(11)
    streams = []
    for i in range(streams_n):
        rate, fmt = MIX[i % len(MIX)]
        pieces = [(torch.randn(48000 + 256 * i, generator=g) * 0.1).to(DEV) for _ in range(3)]
        fades = [0, 3600, 3600]
        total = I.join_plan([p.shape[0] for p in pieces], fades)[2]
        settled = total - 3600
        streams.append(dict(pieces=pieces, fades=fades, settled=settled, final=False, range=(0, I.deliver_plan(rate, settled, False)[1]),
                            out_rate=rate, sample_format=fmt))

    def emit():
        return I.wave_emit(model.mel_spec, streams)[0]

    def chain():
        return [I.wave_deliver(model.mel_spec, [I.wave_join(s["pieces"], s["fades"])[:s["settled"]]], out_rate=s["out_rate"],
                               sample_format=s["sample_format"], ranges=[s["range"]], final=False)[0] for s in streams]

    times = {"emit": [], "chain": []}
    same = True
    for r in range(runs + 2):
        for name, fn in (("emit", emit), ("chain", chain)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            if r >= 2:
                times[name].append((time.perf_counter() - t0) * 1e3)
            if name == "emit":
                kept = out
            else:
                same = same and all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(kept, out))
    return {"streams": streams_n, "pieces": 3 * streams_n, "emit_ms": spread(times["emit"]), "chain_ms": spread(times["chain"]),
            "chain_launches": 2 * streams_n, "emit_equals_chain_bits": same}


def save(rec, path):
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            fh.write(json.dumps(rec) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--clients", default="1,4,16")
    ap.add_argument("--nfe", type=int, default=16)
    ap.add_argument("--precision", default="f16p")
    ap.add_argument("--granule", type=int, default=64)
    ap.add_argument("--batch-frames", type=int, default=40000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pool_time.py measures on the GPU: none is visible")

    tr = P.DiT(**P.config.F5TTS_BASE, text_num_embeds=P.config.VOCAB_SIZE + 1, mel_dim=100, precision=args.precision).init_synthetic(seed=0)
    model = P.CFM(transformer=tr, mel_spec_module=P.mel.MelSpec()).to(DEV)
    voc = P.Vocos(P.config.VOCOS_24K).init_synthetic(seed=1).to(DEV)
    tr.set_length_buckets(args.granule)
    audio = torch.randn(1, 240000, generator=torch.Generator().manual_seed(5)) * 0.05
    kw = dict(nfe_step=args.nfe, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=0)
    bank = I.prepare_voices(model, {"main": dict(ref_audio=(audio, 24000), ref_text=REF_TEXT)})
    chunks = I.stream_chunks(TEXT, REF_TEXT, 10.0, True)
    assert len(REF_TEXT.encode()) == 100 and [c.count(".") for c in chunks] == [1, 1, 2, 4, 4, 4], chunks

    rec = {"tool": "pool_time", "precision": args.precision, "nfe": args.nfe, "granule": args.granule, "runs": args.runs,
           "batch_frames": args.batch_frames, "chunks": len(chunks), "clocks": "host perf_counter to packet arrival / leg end; emit: host clock around calls + device synchronise",
           "clients": {}}
    for K in [int(k) for k in args.clients.split(",")]:
        mix = [MIX[i % len(MIX)] for i in range(K)]
        sessions = [I.open_stream(model, voc, (bank, "main"), out_rate=rate, sample_format=fmt, lookahead=1, **kw) for rate, fmt in mix]
        pool = I.open_pool(model, voc, bank, batch_frames=args.batch_frames, **kw)
        clients = [pool.connect("main", out_rate=rate, sample_format=fmt) for rate, fmt in mix]
        legs = {"sessions": lambda: run_sessions(sessions), "pool": lambda: run_pool(pool, clients)}
        times = {name: [] for name in legs}
        ticks_before = 0
        for r in range(args.runs + 2):
            for name, leg in legs.items():
                firsts, total, counts = leg()
                torch.cuda.synchronize()
                audio_s = sum(n / rate for n, (rate, _) in zip(counts, mix))
                if r >= 2:
                    times[name].append((audio_s / (total / 1e3), statistics.median(firsts), max(firsts), total))
            if r == 1:
                ticks_before = pool.stats()["ticks"]
        out = {"audio_seconds_per_round": round(audio_s, 2), "pool_ticks_per_round": (pool.stats()["ticks"] - ticks_before) / args.runs,
               "pool_rows_per_tick": [len(t) for t in pool.log[-int((pool.stats()["ticks"] - ticks_before) / args.runs):]]}
        for name, ts in times.items():
            out[name] = {"audio_s_per_wall_s": spread([t[0] for t in ts]), "first_packet_ms_median_client": spread([t[1] for t in ts]),
                         "first_packet_ms_worst_client": spread([t[2] for t in ts]), "total_ms": spread([t[3] for t in ts])}
        rec["clients"][str(K)] = out
        save(rec, args.out)
        print(f"K = {K:3d}  sessions {out['sessions']['audio_s_per_wall_s']['median']:8.2f} audio-s/s, first packet worst "
              f"{out['sessions']['first_packet_ms_worst_client']['median']:9.1f} ms   pool {out['pool']['audio_s_per_wall_s']['median']:8.2f} audio-s/s, "
              f"first packet worst {out['pool']['first_packet_ms_worst_client']['median']:9.1f} ms", flush=True)
    rec["emit_against_chain"] = emit_against_chain(model, args.runs)
    rec["graph_stats"] = tr.graph_stats()
    print(json.dumps(rec))
    save(rec, args.out)


if __name__ == "__main__":
    main()
