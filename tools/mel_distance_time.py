"""Cost of the DTW-aligned mel-cepstral distance (f5_mel_distance, csrc/dtw.hip):

  (1) the device call -- HIP events around one call, median of --reps calls after a warm-up -- for three sets of pairs:
      c3     32 pairs with the lengths of bench.py's C3 batch (N_i ~ U{384..1024} seed 1234, the generated 3/4 of each against a
             recording 0.9 .. 1.1 times as long);
      short  64 pairs of 60 .. 200 frames;
      long   one 4096 x 4096 pair (a single workgroup: about 8,000 barrier steps);
      beside the NumPy float64 restatement of the contract (tests/dtw_oracle.py) on the host for the same pairs, timed once: what a
      user would run without this call.  The device results are checked against it (relative 2^-39) while it is there;
  (2) infer.heldout_distance for 32 items at F5-TTS Base size (synthetic weights), NFE 16, wall time ending in a synchronise,
      beside the same sample() calls alone: the share of the walk that is sample().

    python tools/mel_distance_time.py [--precision f16p] [--reps 30] [--no-host] [--no-model]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dtw_oracle as O  # noqa: E402
import f5_tts_amd as P  # noqa: E402

DEV = "cuda:0"


def c3_lengths(count=32):
    gl = torch.Generator().manual_seed(1234)
    return [1024] + [int(x) for x in torch.randint(384, 1025, (count - 1,), generator=gl)]


def pair_sets():
    g = np.random.default_rng(0)
    gen = [n - n // 4 for n in c3_lengths()]
    return {"c3": [(n, int(round(n * g.uniform(0.9, 1.1)))) for n in gen],
            "short": [(int(g.integers(60, 201)), int(g.integers(60, 201))) for _ in range(64)],
            "long": [(4096, 4096)]}


def median_ms(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times), max(times)


def time_pairs(args):
    for name, shapes in pair_sets().items():
        pairs = [O.pair(17 * k + n, n, m) for k, (n, m) in enumerate(shapes)]
        a = [torch.from_numpy(x).to(DEV) for x, _ in pairs]
        b = [torch.from_numpy(y).to(DEV) for _, y in pairs]
        med, lo, hi = median_ms(lambda: P.metrics.mel_distance(a, b), args.reps)
        cells = sum(n * m for n, m in shapes)
        line = (f"{name}: {len(shapes)} pairs, {cells / 1e6:.2f} M cells: f5_mel_distance {med:.3f} ms per call (median of {args.reps}, "
                f"min {lo:.3f}, max {hi:.3f}; HIP events, host staging of the tables included)")
        if not args.no_host:
            got = P.metrics.mel_distance(a, b).cpu().tolist()
            t0 = time.perf_counter()
            want = [O.value(x, y) for x, y in pairs]
            host = time.perf_counter() - t0
            worst = max(abs(g - w) / w for g, w in zip(got, want))
            assert worst <= 2.0 ** -39, worst
            line += f"; NumPy float64 on the host {host * 1e3:.0f} ms (once); device against it: max relative {worst:.1e}"
        print(line, flush=True)


def time_driver(args):
    arch, nv = P.config.F5TTS_BASE, P.config.VOCAB_SIZE + 1
    sd = P.weights.synthetic_state_dict(P.weights.dit_param_shapes(arch, nv))
    tr = P.DiT(**arch, text_num_embeds=nv, mel_dim=100, precision=args.precision)
    tr.load_state_dict(sd)
    model = P.CFM(transformer=tr, mel_spec_module=P.mel.MelSpec()).to(DEV)
    g = torch.Generator().manual_seed(1)
    items = []
    for k, n in enumerate(c3_lengths()):
        p = n // 4
        whole = torch.from_numpy(O.random_walk_mel(100 + k, n))
        items.append((whole[:p].clone(), torch.randint(1, nv - 2, (round(0.04 * n),), generator=g), whole[p:].clone(),
                      torch.randint(1, nv - 2, (round(0.11 * n),), generator=g)))
    kw = dict(nfe_step=16, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=0)
    texts, lens, totals, groups = P.infer.heldout_distance_plan(items)
    pad = torch.nn.utils.rnn.pad_sequence

    def samples_alone():
        for run in groups:
            cond = pad([items[u][0] for u in run], batch_first=True).to(DEV)
            text = pad([torch.tensor(texts[u]) for u in run], padding_value=-1, batch_first=True)
            model.sample(cond, text, torch.tensor([totals[u] for u in run]), lens=torch.tensor([lens[u] for u in run]), steps=16,
                         cfg_strength=2.0, sway_sampling_coef=-1.0, seed=0)
        torch.cuda.synchronize()

    def scored():
        r = P.infer.heldout_distance(model, items, **kw)
        torch.cuda.synchronize()
        return r

    res = None
    for _ in range(2):          # arena growth, graph capture, first replay
        samples_alone()
        res = scored()
    walls = {"sample": [], "scored": []}
    for _ in range(5):          # alternating, so that both see the same machine
        t0 = time.perf_counter()
        samples_alone()
        walls["sample"].append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        scored()
        walls["scored"].append(time.perf_counter() - t0)
    s, d = statistics.median(walls["sample"]), statistics.median(walls["scored"])
    print(f"heldout_distance, {len(items)} items in {len(groups)} batches at F5-TTS Base {args.precision}, NFE 16: {d * 1e3:.0f} ms of wall time "
          f"(median of 5), the same sample() calls alone {s * 1e3:.0f} ms: sample() is {100 * s / d:.1f} % of the walk "
          f"(mcd {res[None]['mcd']:.4f} dB on synthetic weights)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="f16p")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--no-host", action="store_true", help="skip the NumPy restatement on the host")
    ap.add_argument("--no-model", action="store_true", help="skip part (2)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mel_distance_time needs a GPU: a time taken anywhere else says nothing about it")
    time_pairs(args)
    if not args.no_model:
        time_driver(args)


if __name__ == "__main__":
    main()
