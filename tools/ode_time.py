"""ms per CFM.sample() at the C2 shape (F5-TTS Base, B=1, N=1024, prompt 256 frames, 154 text ids, cfg 2, sway -1,
synthetic weights) for the fixed-grid ODE solvers: Euler at 16 steps and midpoint at 8 and 16 steps (NFE 16 / 16 / 32).

    python tools/ode_time.py [--precision f16p] [--reps 10]

Each configuration runs twice untimed (eager, then HIP-graph capture) and is then timed as graph replays with HIP events
around each sample() call; the median is printed.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import f5_tts_amd as P  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="f16p")
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    arch = P.config.F5TTS_BASE
    nv = P.config.VOCAB_SIZE + 1
    tr = P.DiT(**arch, text_num_embeds=nv, mel_dim=100, precision=args.precision)
    tr.load_state_dict(P.weights.synthetic_state_dict(P.weights.dit_param_shapes(arch, nv)))
    model = P.CFM(transformer=tr, mel_spec_module=P.mel.MelSpec()).to("cuda:0")
    model.transformer.engine().reserve(1, 1024, 16)
    g = torch.Generator().manual_seed(1)
    cond = torch.randn(1, 256, 100, generator=g)
    text = torch.randint(1, P.config.VOCAB_SIZE - 1, (1, 154), generator=g)
    res = {}
    for method, steps in (("euler", 16), ("midpoint", 8), ("midpoint", 16)):
        model.odeint_kwargs = dict(method=method)
        kw = dict(steps=steps, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=0)
        for _ in range(2):
            model.sample(cond, text, 1024, **kw)
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            model.sample(cond, text, 1024, **kw)
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        res[(method, steps)] = statistics.median(ms)
        nfe = steps * (2 if method == "midpoint" else 1)
        print(f"{args.precision} {method:8s} steps {steps:2d} (NFE {nfe:2d}): {res[(method, steps)]:8.2f} ms per sample() "
              f"(median of {args.reps}; min {min(ms):.2f})", flush=True)
    e16 = res[("euler", 16)]
    print(f"midpoint 16 / euler 16 = {res[('midpoint', 16)] / e16:.3f};  midpoint 8 / euler 16 = {res[('midpoint', 8)] / e16:.3f}")


if __name__ == "__main__":
    main()
