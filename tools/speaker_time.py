"""Cost of the Gaussian cepstral divergence (f5_cep_moments, f5_gauss_divergence, csrc/speaker.hip):

  (1) the device calls -- HIP events around one call, median of --reps calls after a warm-up -- on 32 synthetic log-mels with the
      lengths of bench.py's C3 batch (four synthetic speakers, eight items each; tests/speaker_oracle.py's construction):
      cepstral_moments without and with deltas, gaussian_divergence of the 32 records against a shifted copy, merge_moments by
      speaker; beside the ordered NumPy float64 oracle on the host for the same 32 items, timed once, with the device result checked
      against it while it is there (equal);
  (2) how the pooled numbers move with the gate on this set: same-speaker and different-speaker kl and sphericity of the pooled
      records at gate_db None, 40, 30, 20, 10 -- an observation about synthetic data, not a recommendation.

    python tools/speaker_time.py [--reps 30] [--no-host]
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import speaker_oracle as O  # noqa: E402
import f5_tts_amd as P  # noqa: E402
from mel_distance_time import c3_lengths, median_ms  # noqa: E402

DEV = "cuda:0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--no-host", action="store_true", help="skip the NumPy oracle on the host")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("speaker_time needs a GPU: a time taken anywhere else says nothing about it")
    M = P.metrics
    rng = np.random.default_rng(0)
    voices = [O.synthetic_speaker(rng) for _ in range(4)]
    lens = c3_lengths()
    who = [k % 4 for k in range(len(lens))]
    host = [O.synthetic_utterance(rng, voices[w], n) for w, n in zip(who, lens)]
    mels = [torch.from_numpy(x).to(DEV) for x in host]
    plain, wide = M.cepstral_moments(mels), M.cepstral_moments(mels, deltas=True)
    shifted = [(k + 4) % len(lens) for k in range(len(lens))]       # the same speaker's next item
    what = {"cepstral_moments (13 cepstra)": lambda: M.cepstral_moments(mels),
            "cepstral_moments (13 cepstra and deltas)": lambda: M.cepstral_moments(mels, deltas=True),
            "gaussian_divergence (C = 13, 32 pairs)": lambda: M.gaussian_divergence(plain, plain, list(enumerate(shifted))),
            "gaussian_divergence (C = 26, 32 pairs)": lambda: M.gaussian_divergence(wide, wide, list(enumerate(shifted))),
            "merge_moments (32 records, 4 speakers; torch ops)": lambda: M.merge_moments(plain, who)}
    print(f"{len(lens)} items, {sum(lens)} frames, longest {max(lens)}; workspace {M.cepstral_moments_plan(lens, deltas=True)} bytes with "
          f"deltas", flush=True)
    for name, fn in what.items():
        med, lo, hi = median_ms(fn, args.reps)
        print(f"{name}: {med:.3f} ms per call (median of {args.reps}, min {lo:.3f}, max {hi:.3f}; HIP events, host staging included)",
              flush=True)
    if not args.no_host:
        t0 = time.perf_counter()
        want = [O.moments(x, 13, True) for x in host]
        took_m = time.perf_counter() - t0
        t0 = time.perf_counter()
        terms = [O.divergence(want[i], want[j])[0] for i, j in enumerate(shifted)]
        took_d = time.perf_counter() - t0
        got_t, _ = M.gaussian_divergence(wide, wide, list(enumerate(shifted)))
        same = (np.array_equal(wide.scatter.cpu().numpy(), np.stack([w[2] for w in want]))
                and np.array_equal(wide.mean.cpu().numpy(), np.stack([w[1] for w in want]))
                and np.array_equal(got_t.cpu().numpy(), np.array(terms)))
        assert same
        print(f"ordered NumPy float64 oracle on the host (once): moments with deltas {took_m * 1e3:.0f} ms, 32 divergences at C = 26 "
              f"{took_d * 1e3:.0f} ms; device results equal: {same}", flush=True)
    # how the pooled numbers move with the gate (synthetic data: an observation, not a recommendation)
    halves = [f"{w}{'ab'[(k // 4) % 2]}" for k, w in enumerate(who)]  # every speaker's items in two disjoint pools
    labels = sorted(set(halves))
    for gate_db in (None, 40.0, 30.0, 20.0, 10.0):
        rec = M.cepstral_moments(mels, gate_db=gate_db)
        pooled, names = M.merge_moments(rec, halves)
        idx = {n: k for k, n in enumerate(names)}
        same_pairs = [(idx[f"{w}a"], idx[f"{w}b"]) for w in range(4)]
        other_pairs = [(idx[f"{w}a"], idx[f"{(w + 1) % 4}b"]) for w in range(4)]
        terms, status = M.gaussian_divergence(pooled, pooled, same_pairs + other_pairs)
        nums = M.speaker_numbers(terms.cpu(), 13)
        kept = int(rec.count.clamp(min=0).sum())
        print(f"gate_db {gate_db}: {kept} of {sum(lens)} frames kept, {len(labels)} pools; same speaker kl {np.mean(nums['kl'][:4]):.4f} "
              f"sphericity {np.mean(nums['sphericity'][:4]):.5f}; other speaker kl {np.mean(nums['kl'][4:]):.2f} sphericity "
              f"{np.mean(nums['sphericity'][4:]):.4f}; singular {int(status.sum())}", flush=True)


if __name__ == "__main__":
    main()
