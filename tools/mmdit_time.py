"""What one MMDiT step costs: ms per ODE step, launches per block, and the split between GEMM, attention and LayerNorm.

    python tools/mmdit_time.py [--runs 30] [--precisions f16p,f16x3] [--out FILE.json]

dim 1024, depth 8, heads 16, ff_mult 2, synthetic weights; B = 1, N = 1000 frames (a 256-frame prompt), nt = 200 tokens, NFE 16,
cfg 2, sway -1.  Timed: CFM.sample with graphs on (the timed calls replay) -- a device synchronise, a host clock around the call and
a device synchronise; two warm-up calls, the median of --runs with min - max, divided by the 16 steps.  Then one call with the
engine's per-launch profiler (eager launches, one event pair per launch): launches and milliseconds per class, per step; the
launches per block are (gemm + attention + layernorm + misc launches of the blocks) / (steps x evaluations x depth).  No speed is
claimed for this backbone; the numbers go to DESIGN.md."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import f5_tts_amd as P  # noqa: E402

DEV = "cuda:0"
ARCH = dict(dim=1024, depth=8, heads=16, dim_head=64, ff_mult=2)
N, PROMPT, NT, NFE = 1000, 256, 200, 16


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def measure(precision, runs):
    tr = P.MMDiT(**ARCH, text_num_embeds=2546, mel_dim=100, precision=precision).init_synthetic()
    model = P.CFM(transformer=tr, mel_spec_module=P.mel.MelSpec()).to(DEV)
    g = torch.Generator().manual_seed(3)
    cond = torch.randn(1, PROMPT, 100, generator=g).to(DEV)
    text = torch.randint(0, 2000, (1, NT), generator=g)

    def call():
        return model.sample(cond, text, N, steps=NFE, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=0)

    for _ in range(3):   # eager, capture, first replay
        call()
    ms = [timed(call) for _ in range(runs)]
    eng = tr.engine()
    eng.profile(True)
    call()
    prof = eng.profile_read()
    eng.profile(False)
    depth = ARCH["depth"]
    # per forward outside the blocks: 1 input GEMM + 1 output GEMM, 1 final LayerNorm, 1 pack + (no lengths at B = 1) 0 misc
    evals = NFE * 1
    gemm_blocks = prof["gemm"]["launches"] - 2 * evals   # (the time path's GEMMs are in its own class)
    ln_blocks = prof["layernorm"]["launches"] - evals
    misc_blocks = prof["misc"]["launches"] - 2 * evals - 2 - NFE  # pack + V^T zero per forward; the two select_rows; one Euler update per step
    per_block = (gemm_blocks + prof["attention"]["launches"] + ln_blocks + misc_blocks) / (evals * depth)
    total = sum(v["ms"] for v in prof.values())
    return dict(precision=precision, ms_per_step=round(statistics.median(ms) / NFE, 3),
                ms_per_step_min_max=[round(min(ms) / NFE, 3), round(max(ms) / NFE, 3)], launches_per_block=round(per_block, 2),
                profile_ms_per_step={k: round(v["ms"] / NFE, 3) for k, v in prof.items()},
                profile_share={k: round(v["ms"] / total, 3) for k, v in prof.items() if k in ("gemm", "attention", "layernorm")},
                launches={k: v["launches"] for k, v in prof.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--precisions", default="f16p,f16x3")
    ap.add_argument("--out")
    a = ap.parse_args()
    res = dict(arch=ARCH, B=1, N=N, nt=NT, nfe=NFE, results=[measure(p, a.runs) for p in a.precisions.split(",")])
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
