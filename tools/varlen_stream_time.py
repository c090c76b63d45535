"""What a stream of utterances of varying length costs per utterance, with and without length-bucketed sample() graphs.

    python tools/varlen_stream_time.py [--utts 26] [--granule 64] [--nfe 16] [--precision f16p] [--out FILE.json]

F5-TTS Base, B = 1, cfg 2.0, EPSS + sway grid; `--utts` utterances with DISTINCT lengths drawn the way bench.py draws its
seed-1234 lengths (N ~ U{384..1024}, prompt N // 4 frames, round(0.15 N) text ids), each seen once per leg, one process:

  (a) buckets off      -- every call is a new exact shape: eager launches (the behaviour of a serving stream today)
  (b) granule G        -- after prepare_sample() over the stream's range: every call replays the graph of its bucket
  (c) floor            -- every N as a warmed replay of its own exact-shape graph (what a repeated shape costs)

Per leg: wall time per utterance (host clock around CFM.sample + a device synchronise), audio seconds / wall second and
f5_graph_stats; prepare_sample()'s own wall time; and the text-encoder class of one profiled call (f5_profile_read), which is what
computing the unconditional text embedding inside every bucketed body costs.  Prints a per-length table and one JSON line.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import f5_tts_amd as P  # noqa: E402

DEV = "cuda:0"


def draw_lengths(n_utts):
    """bench.py make_c4_job's generator, keeping the first n_utts distinct draws."""
    gl = torch.Generator().manual_seed(1234)
    durs = []
    while len(durs) < n_utts:
        d = int(torch.randint(384, 1025, (1,), generator=gl))
        if d not in durs:
            durs.append(d)
    return durs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=26)
    ap.add_argument("--granule", type=int, default=64)
    ap.add_argument("--nfe", type=int, default=16)
    ap.add_argument("--precision", default="f16p")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("varlen_stream_time.py measures on the GPU: none is visible")

    durs = draw_lengths(args.utts)
    g = torch.Generator().manual_seed(1)
    conds = [torch.randn(1, d // 4, 100, generator=g).to(DEV) for d in durs]
    texts = [torch.randint(1, P.config.VOCAB_SIZE - 1, (1, round(0.15 * d)), generator=g) for d in durs]
    audio_s = sum((d - d // 4) * P.config.HOP_LENGTH / P.config.SAMPLE_RATE for d in durs)
    kw = dict(steps=args.nfe, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=0)

    def build():
        tr = P.DiT(**P.config.F5TTS_BASE, text_num_embeds=P.config.VOCAB_SIZE + 1, mel_dim=100, precision=args.precision).init_synthetic(seed=0)
        model = P.CFM(transformer=tr, mel_spec_module=P.mel.MelSpec()).to(DEV)
        tr.engine().reserve(1, 1024, args.nfe)
        return tr, model

    def call(model, i):
        t0 = time.perf_counter()
        out, _ = model.sample(conds[i], texts[i], durs[i], **kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def warm_code_objects(model):
        """Loads every kernel at a length outside the stream, so that no leg pays for first launches."""
        for _ in range(2):
            model.sample(conds[0][:, :80], texts[0][:, :48], 320, **kw)
        torch.cuda.synchronize()

    def leg(model, tr):
        tr.graph_stats(reset=True)
        ms, outs = [], []
        for i in range(len(durs)):
            t, out = call(model, i)
            ms.append(t)
            outs.append(out)
        return ms, outs, tr.graph_stats()

    # ---- (a) buckets off, each N once
    tr, model = build()
    warm_code_objects(model)
    ms_a, outs_a, st_a = leg(model, tr)
    # the text encoder of one call (conditional + unconditional embedding), from the engine's profiler
    eng = tr.engine()
    eng.profile(True)
    call(model, 0)
    text_cls = eng.profile_read()["text_encoder"]
    eng.profile(False)

    # ---- (b) granule G, graphs prepared ahead of the stream
    tr.set_length_buckets(args.granule)
    t0 = time.perf_counter()
    tr.prepare_sample(1, min(durs), max(durs), max(t.shape[1] for t in texts), args.nfe, 2.0)
    torch.cuda.synchronize()
    prepare_ms = (time.perf_counter() - t0) * 1e3
    st_prep = tr.graph_stats()
    ms_b, outs_b, st_b = leg(model, tr)
    same = all(torch.equal(x, y) for x, y in zip(outs_a, outs_b))

    # ---- (c) the floor: each N as a warmed replay of its own exact-shape graph
    tr.set_length_buckets(0)
    ms_c = []
    for i in range(len(durs)):
        for _ in range(3):   # eager (stores the unconditional text embedding), capture, replay
            call(model, i)
        ms_c.append(call(model, i)[0])
    st_c = tr.graph_stats()

    ceil = [-(-d // args.granule) * args.granule for d in durs]
    print(f"{'N':>5} {'N_cap':>5} {'pad %':>6} {'(a) off ms':>11} {'(b) bucket ms':>13} {'(c) floor ms':>12} {'b/c':>6}")
    for d, c, a, b, f in sorted(zip(durs, ceil, ms_a, ms_b, ms_c)):
        print(f"{d:5d} {c:5d} {100.0 * (c - d) / d:6.1f} {a:11.2f} {b:13.2f} {f:12.2f} {b / f:6.3f}")
    rec = {
        "tool": "varlen_stream_time", "precision": args.precision, "nfe": args.nfe, "granule": args.granule, "utterances": len(durs),
        "lengths": durs, "audio_seconds": round(audio_s, 3), "bucket_results_equal_exact_path": same,
        "prepare_sample_ms": round(prepare_ms, 1), "prepare_sample_stats": st_prep,
        "text_encoder_ms_per_call_cond_plus_uncond": round(text_cls["ms"], 3), "text_encoder_launches": text_cls["launches"],
    }
    for name, ms, st in (("a_buckets_off", ms_a, st_a), ("b_bucketed_prepared", ms_b, st_b), ("c_exact_shape_replay_floor", ms_c, st_c)):
        rec[name] = {"ms_per_utterance_mean": round(sum(ms) / len(ms), 3), "ms_per_utterance_max": round(max(ms), 3),
                     "ms_per_utterance": [round(x, 2) for x in ms], "audio_s_per_wall_s": round(audio_s / (sum(ms) / 1e3), 1),
                     "graph_stats": st}
    rec["b_over_c"] = round(sum(ms_b) / sum(ms_c), 4)
    rec["a_over_c"] = round(sum(ms_a) / sum(ms_c), 4)
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
