"""f8 against f16 / f16p of this tree, in one process (medians of 30 repeats, the two precisions alternating inside every repeat):

  * the four block GEMMs at Base dims (QKV 1024 -> 3072, out 1024 -> 1024, FF1 1024 -> 2048, FF2 2048 -> 1024) at 2,048 and 32,768
    rows through f5k_gemm_time: f16 operands, e4m3 operands, and e4m3 operands with the stand-alone quantise launch of an f16 A
    operand in the timed region (what the engine pays in front of the out-projection and FF2; QKV and FF1 get their codes from the
    LayerNorm, whose e4m3 form replaces the f16 form launch for launch);
  * sample() at the C2 shape (Base, B = 1, 256 + 768 frames, NFE 16, cfg 2) and at a C3-like shape (B = 16 x 1,000 frames, NFE 16),
    f16p against f8, device-synchronised host clock around each call, graphs on (the first calls capture and are not timed).

usage: python tools/f8_time.py [--gemm-only | --sample-only]
"""
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import f5_tts_amd as P  # noqa: E402
from f5_tts_amd import _lib  # noqa: E402

DEV = "cuda:0"
REPEATS = 30
GEMMS = (("qkv", 3072, 1024), ("out", 1024, 1024), ("ff1", 2048, 1024), ("ff2", 1024, 2048))


def gemm_us(prec, M, N, K, with_quant=False, iters=8):
    us = C.c_float(0)
    _lib.check(_lib.load().f5k_gemm_time(_lib.PRECISIONS[prec], M, N, K, 0, 1 if with_quant else 0, iters, C.byref(us),
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream)), "f5k_gemm_time")
    return us.value


def time_gemms():
    for M in (2048, 32768):
        tot = {"f16": 0.0, "f8": 0.0, "f8+q": 0.0}
        for name, N, K in GEMMS:
            runs = {k: [] for k in tot}
            for _ in range(REPEATS):   # alternating: f16, f8, f8 + quantise
                runs["f16"].append(gemm_us("f16", M, N, K))
                runs["f8"].append(gemm_us("f8", M, N, K))
                runs["f8+q"].append(gemm_us("f8", M, N, K, with_quant=True))
            med = {k: statistics.median(v) for k, v in runs.items()}
            fl = 2.0 * M * N * K
            print(f"rows {M:6d} {name}: f16 {med['f16']:7.1f} us ({fl / med['f16'] / 1e6:5.0f} TF) | f8 {med['f8']:7.1f} us "
                  f"({fl / med['f8'] / 1e6:5.0f} TF, {med['f16'] / med['f8']:.2f}x) | f8 + quantise {med['f8+q']:7.1f} us "
                  f"({med['f16'] / med['f8+q']:.2f}x)", flush=True)
            for k in tot:
                tot[k] += med[k]
        print(f"rows {M:6d} four GEMMs: f16 {tot['f16']:7.1f} us | f8 {tot['f8']:7.1f} us ({tot['f16'] / tot['f8']:.2f}x) | f8 with a quantise "
              f"launch in front of each {tot['f8+q']:7.1f} us ({tot['f16'] / tot['f8+q']:.2f}x)", flush=True)


def model(prec):
    NV = P.config.VOCAB_SIZE + 1
    arch = P.config.F5TTS_BASE
    tr = P.DiT(**arch, text_num_embeds=NV, mel_dim=100, precision=prec)
    tr.load_state_dict(P.weights.synthetic_state_dict(P.weights.dit_param_shapes(arch, NV)))
    return P.CFM(transformer=tr, mel_spec_module=P.mel.MelSpec()).to(DEV), NV


def time_sample():
    models = {p: model(p) for p in ("f16p", "f8")}
    g = torch.Generator().manual_seed(1)
    for label, B, ref, N in (("C2 (B = 1, 1,024 frames, NFE 16)", 1, 256, 1024), ("C3-like (B = 16 x 1,000 frames, NFE 16)", 16, 250, 1000)):
        NV = models["f8"][1]
        cond = torch.randn(B, ref, 100, generator=g)
        text = torch.randint(1, NV - 2, (B, round(0.15 * N)), generator=g)
        kw = dict(steps=16, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=0)
        if B > 1:
            kw["lens"] = torch.full((B,), ref)
        dur = N if B == 1 else torch.full((B,), N)
        runs = {p: [] for p in models}
        for p, (m, _) in models.items():
            for _ in range(3):   # capture + warm
                m.sample(cond, text, dur, **kw)
        torch.cuda.synchronize()
        for _ in range(REPEATS):
            for p, (m, _) in models.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                m.sample(cond, text, dur, **kw)
                torch.cuda.synchronize()
                runs[p].append((time.perf_counter() - t0) * 1e3)
        med = {p: statistics.median(v) for p, v in runs.items()}
        print(f"sample() {label}: f16p {med['f16p']:.2f} ms | f8 {med['f8']:.2f} ms ({med['f16p'] / med['f8']:.3f}x)  "
              f"[min f16p {min(runs['f16p']):.2f}, f8 {min(runs['f8']):.2f}]", flush=True)


if __name__ == "__main__":
    torch.zeros(1, device=DEV)
    if "--sample-only" not in sys.argv:
        time_gemms()
    if "--gemm-only" not in sys.argv:
        time_sample()
