"""Cost of the smoothed pitch tracks (f5_pitch_candidates, f5_pitch_decode, csrc/pitch.hip):

  (1) the device calls -- HIP events around one call, median of --reps calls after a warm-up -- on 32 waves with the lengths of
      bench.py's C3 batch (tools/prosody_time.py's waves) at the defaults (window 1024, lags 40 .. 400, 100 thresholds, 202 bins):
      pitch_candidates, pitch_decode on its output, the whole pitch_track_pyin, and pitch_track (YIN) in the same process;
      beside the NumPy float64 restatement of the contract (tests/pyin_oracle.py) on the host for the first 48 frames of the first
      wave, timed once; the device result is checked against it while it is there (equal);
  (2) infer.heldout_prosody for the same 32 items at F5-TTS Base size with a Vocos of full size (synthetic weights), NFE 16, wall
      time ending in a synchronise, with pitch="yin" and with pitch="pyin", alternating.

    python tools/pyin_time.py [--precision f16p] [--reps 30] [--no-host] [--no-model]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import dtw_oracle as O  # noqa: E402
import pyin_oracle as Q  # noqa: E402
import f5_tts_amd as P  # noqa: E402
from mel_distance_time import c3_lengths, median_ms  # noqa: E402
from prosody_time import voiced_wave  # noqa: E402

DEV = "cuda:0"
HOP = 256


def time_tracks(args):
    M = P.metrics
    lens = [(n - n // 4 - 1) * HOP for n in c3_lengths()]
    host = [voiced_wave(n, 7 * k + 1) for k, n in enumerate(lens)]
    waves = [torch.from_numpy(x).to(DEV) for x in host]
    tab = M.pyin_tables()
    frames = sum(n // HOP + 1 for n in lens)
    count, _, f0, prob, fr = M.pitch_candidates(waves, tables=tab)
    what = {"pitch_candidates": lambda: M.pitch_candidates(waves, tables=tab),
            "pitch_decode": lambda: M.pitch_decode(count, f0, prob, fr, tab),
            "pitch_track_pyin": lambda: M.pitch_track_pyin(waves, tables=tab),
            "pitch_track (YIN)": lambda: M.pitch_track(waves)}
    print(f"{len(lens)} waves, {frames} frames ({sum(lens) / 24000:.0f} s of audio), {tab.n} thresholds, {tab.bins} bins, reach {tab.reach}; "
          f"longest item {max(fr)} frames; {int(count.sum())} candidates, at most {int(count.max())} in a frame", flush=True)
    for name, fn in what.items():
        med, lo, hi = median_ms(fn, args.reps)
        print(f"{name}: {med:.3f} ms per call (median of {args.reps}, min {lo:.3f}, max {hi:.3f}; HIP events, host staging of the tables "
              f"included)", flush=True)
    if args.no_host:
        return
    n = 48
    x = host[0][:(n - 1) * HOP]
    g0, gv, _ = M.pitch_track_pyin([torch.from_numpy(x).to(DEV)], tables=tab)
    otab = Q.tables(tau_min=tab.tau_min, tau_max=tab.tau_max)
    t0 = time.perf_counter()
    w0, wv = Q.track(x, otab, window=1024, frames=n)
    took = time.perf_counter() - t0
    same = np.array_equal(g0.cpu().numpy(), w0) and np.array_equal(gv.cpu().numpy(), wv)
    assert same
    print(f"NumPy float64 on the host: {took * 1e3:.0f} ms for {n} frames (once: {took / n * frames:.0f} s for all at that rate); device "
          f"track equal: {same}", flush=True)


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

    def scored(pitch):
        r = P.infer.heldout_prosody(model, voc, items, pitch=pitch, **kw)
        torch.cuda.synchronize()
        return r

    res = {}
    for _ in range(2):          # arena growth, graph capture, first replay
        for pitch in ("yin", "pyin"):
            res[pitch] = scored(pitch)[None]
    walls = {"yin": [], "pyin": []}
    for _ in range(5):          # alternating, so that both see the same machine
        for pitch in walls:
            t0 = time.perf_counter()
            scored(pitch)
            walls[pitch].append(time.perf_counter() - t0)
    y, p = statistics.median(walls["yin"]), statistics.median(walls["pyin"])
    print(f"heldout_prosody, {len(items)} items at F5-TTS Base {args.precision} with Vocos, NFE 16, wall time (median of 5): pitch='yin' "
          f"{y * 1e3:.0f} ms, pitch='pyin' {p * 1e3:.0f} ms", flush=True)
    for pitch, r in res.items():
        print(f"  {pitch} (synthetic weights): mcd {r['mcd']:.4f} dB, f0_rmse_cents {r['f0_rmse_cents']}, f0_corr {r['f0_corr']}, vuv_error "
              f"{r['vuv_error']:.3f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="f16p")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--no-host", action="store_true", help="skip the NumPy restatement on the host")
    ap.add_argument("--no-model", action="store_true", help="skip part (2)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pyin_time needs a GPU: a time taken anywhere else says nothing about it")
    time_tracks(args)
    if not args.no_model:
        time_driver(args)


if __name__ == "__main__":
    main()
