"""Cost of the prosody score (f5_pitch_track, csrc/pitch.hip; f5_mel_align, csrc/dtw.hip):

  (1) the two device calls -- HIP events around one call, median of --reps calls after a warm-up:
      pitch_track   32 waves with the lengths of bench.py's C3 batch (the generated 3/4 of N_i ~ U{384..1024} frames, seed 1234, at
                    256 samples a frame), and one wave of 4096 frames;
      mel_alignment the three sets of tools/mel_distance_time.py (c3, short, long: one 4096 x 4096 pair), beside mel_distance on the
                    same pairs: the difference is the back-pointers and the backtrack;
      beside the NumPy float64 restatements of the contracts (tests/pitch_oracle.py, tests/prosody_oracle.py) on the host for the
      same inputs, timed once; the device results are checked against them while they are there (tracks and paths: equal);
  (2) infer.heldout_prosody for 32 items at F5-TTS Base size with a Vocos of full size (synthetic weights), NFE 16, wall time ending
      in a synchronise, beside the same sample() calls alone: the share of the walk that is sample().

    python tools/prosody_time.py [--precision f16p] [--reps 30] [--no-host] [--no-model]
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
import pitch_oracle as Y  # noqa: E402
import prosody_oracle as R  # noqa: E402
import f5_tts_amd as P  # noqa: E402
from mel_distance_time import c3_lengths, median_ms, pair_sets  # noqa: E402

DEV = "cuda:0"
HOP = 256


def voiced_wave(n, seed):
    g = np.random.default_rng(seed)
    f = g.uniform(90, 260) * (1.0 + 0.08 * np.sin(2 * np.pi * g.uniform(2, 6) * np.arange(n) / 24000.0))
    phase = 2 * np.pi * np.cumsum(f) / 24000.0
    x = sum(np.sin(h * phase + g.uniform(0, 2 * np.pi)) / h for h in (1, 2, 3, 4))
    return (0.25 * x + 0.01 * g.standard_normal(n)).astype(np.float32)


def time_tracks(args):
    sets = {"c3": [(n - n // 4 - 1) * HOP for n in c3_lengths()], "long": [4095 * HOP]}
    for name, lens in sets.items():
        host = [voiced_wave(n, 7 * k + 1) for k, n in enumerate(lens)]
        waves = [torch.from_numpy(x).to(DEV) for x in host]
        med, lo, hi = median_ms(lambda: P.metrics.pitch_track(waves), args.reps)
        frames = sum(n // HOP + 1 for n in lens)
        line = (f"pitch_track {name}: {len(lens)} waves, {frames} frames ({sum(lens) / 24000:.0f} s of audio): {med:.3f} ms per call (median of "
                f"{args.reps}, min {lo:.3f}, max {hi:.3f}; HIP events, host staging of the table included)")
        if not args.no_host:
            f0, ap, fr = P.metrics.pitch_track(waves)
            f0, ap = f0.cpu().numpy(), ap.cpu().numpy()
            few = range(len(host)) if name != "c3" else range(4)            # (the oracle takes seconds per wave)
            t0 = time.perf_counter()
            want = [Y.track(host[k]) for k in few]
            took = time.perf_counter() - t0
            off = np.cumsum([0] + fr)
            worst = max(max(np.abs(f0[off[k]:off[k + 1]] - w0).max(), np.abs(ap[off[k]:off[k + 1]] - wp).max()) for k, (w0, wp) in zip(few, want))
            done = sum(fr[k] for k in few)
            line += (f"; NumPy float64 on the host {took * 1e3:.0f} ms for {done} of the frames (once: {took / done * frames * 1e3:.0f} ms for "
                     f"all at that rate); device against it: max |difference| {worst:.1e}")
        print(line, flush=True)


def time_alignment(args):
    for name, shapes in pair_sets().items():
        pairs = [O.pair(17 * k + n, n, m) for k, (n, m) in enumerate(shapes)]
        a = [torch.from_numpy(x).to(DEV) for x, _ in pairs]
        b = [torch.from_numpy(y).to(DEV) for _, y in pairs]
        med, lo, hi = median_ms(lambda: P.metrics.mel_alignment(a, b), args.reps)
        dmed, _, _ = median_ms(lambda: P.metrics.mel_distance(a, b), args.reps)
        cells = sum(n * m for n, m in shapes)
        line = (f"mel_alignment {name}: {len(shapes)} pairs, {cells / 1e6:.2f} M cells: {med:.3f} ms per call (median of {args.reps}, min {lo:.3f}, "
                f"max {hi:.3f}); mel_distance on the same pairs {dmed:.3f} ms: the path costs {med - dmed:.3f} ms")
        if not args.no_host:
            dist, path, start, plen = P.metrics.mel_alignment(a, b)
            host, lens = path.cpu().tolist(), plen.cpu().tolist()
            few = range(len(pairs)) if name != "c3" else range(4)
            t0 = time.perf_counter()
            want = [R.alignment(*pairs[k])[1] for k in few]
            took = time.perf_counter() - t0
            same = all([tuple(c) for c in host[start[k]:start[k] + lens[k]]] == w for k, w in zip(few, want))
            assert same
            line += f"; NumPy float64 on the host {took * 1e3:.0f} ms for {len(few)} of the pairs (once); device paths equal: {same}"
        print(line, flush=True)


def time_driver(args):
    arch, nv = P.config.F5TTS_BASE, P.config.VOCAB_SIZE + 1
    sd = P.weights.synthetic_state_dict(P.weights.dit_param_shapes(arch, nv))
    tr = P.DiT(**arch, text_num_embeds=nv, mel_dim=100, precision=args.precision)
    tr.load_state_dict(sd)
    model = P.CFM(transformer=tr, mel_spec_module=P.mel.MelSpec()).to(DEV)
    voc = P.Vocos(P.config.VOCOS_24K)
    voc.load_state_dict(P.weights.synthetic_state_dict(P.weights.vocos_param_shapes(P.config.VOCOS_24K), seed=3))
    voc.to(DEV)
    g = torch.Generator().manual_seed(1)
    items = []
    for k, n in enumerate(c3_lengths()):
        p = n // 4
        items.append((torch.from_numpy(O.random_walk_mel(100 + k, p)), torch.randint(1, nv - 2, (round(0.04 * n),), generator=g),
                      torch.from_numpy(voiced_wave((n - p - 1) * HOP, 300 + k)), torch.randint(1, nv - 2, (round(0.11 * n),), generator=g)))
    kw = dict(nfe_step=16, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=0)
    as_mel = [(it[0], it[1], torch.zeros(it[2].numel() // HOP + 1, 100), it[3]) for it in items]
    texts, lens, totals, groups = P.infer.heldout_distance_plan(as_mel)
    pad = torch.nn.utils.rnn.pad_sequence

    def samples_alone():
        for run in groups:
            cond = pad([items[u][0] for u in run], batch_first=True).to(DEV)
            text = pad([torch.tensor(texts[u]) for u in run], padding_value=-1, batch_first=True)
            model.sample(cond, text, torch.tensor([totals[u] for u in run]), lens=torch.tensor([lens[u] for u in run]), steps=16,
                         cfg_strength=2.0, sway_sampling_coef=-1.0, seed=0)
        torch.cuda.synchronize()

    def scored():
        r = P.infer.heldout_prosody(model, voc, items, **kw)
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
    r = res[None]
    print(f"heldout_prosody, {len(items)} items in {len(groups)} batches at F5-TTS Base {args.precision} with Vocos, NFE 16: {d * 1e3:.0f} ms of "
          f"wall time (median of 5), the same sample() calls alone {s * 1e3:.0f} ms: sample() is {100 * s / d:.1f} % of the walk (on synthetic "
          f"weights: mcd {r['mcd']:.4f} dB, f0_rmse_cents {r['f0_rmse_cents']}, f0_corr {r['f0_corr']}, vuv_error {r['vuv_error']:.3f})", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="f16p")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--no-host", action="store_true", help="skip the NumPy restatements on the host")
    ap.add_argument("--no-model", action="store_true", help="skip part (2)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prosody_time needs a GPU: a time taken anywhere else says nothing about it")
    time_tracks(args)
    time_alignment(args)
    if not args.no_model:
        time_driver(args)


if __name__ == "__main__":
    main()
