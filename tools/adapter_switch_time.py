"""Cost of changing the fine-tune an engine serves, at F5-TTS Base size (synthetic weights, the reference recipe's adapter:
rank 16 on to_q / to_k / to_v / to_out.0 of all 22 blocks, rank 64 on input_embed.proj, text encoder replaced):

  (1) f5_set_adapter on the resident engine (F5_OPT_ADAPTERS): device time of one switch (HIP events around `reps`
      switches alternating base <-> adapter), the bytes it reads + writes, and the resulting rate;
  (2) the only other way to change models: a new engine from the host-merged state dict (upload + f5_finalize), wall time;
  (3) for scale, layernorm_kernel on f32 rows (f5k_layernorm_mod at 32,768 x 1,024: 8 bytes per element).

    python tools/adapter_switch_time.py [--precision f16p] [--reps 20]
    rocprofv3 --kernel-trace --stats -- python tools/adapter_switch_time.py --reps 4     # launches per switch, kernel times

Under the profiler adapter_merge_kernel's calls / reps is the number of launches per switch and its average duration the
device time; the event numbers printed here include the launch gaps.
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import f5_tts_amd as P  # noqa: E402
from f5_tts_amd import adapters as A  # noqa: E402

RECIPE = dict(lora_alpha=32, lora_r=16, alpha_pattern={"input_embed.proj": 128}, rank_pattern={"input_embed.proj": 64})


def recipe_adapter(sd, depth, seed=1):
    g = torch.Generator().manual_seed(seed)
    t = {}
    mods = [f"transformer_blocks.{i}.attn.{m}" for i in range(depth) for m in ("to_q", "to_k", "to_v", "to_out.0")] + ["input_embed.proj"]
    for mod in mods:
        w = sd[mod + ".weight"]
        r = 64 if mod == "input_embed.proj" else 16
        t[mod + ".lora_A.weight"] = torch.randn(r, w.shape[1], generator=g) * 0.02
        t[mod + ".lora_B.weight"] = torch.randn(w.shape[0], r, generator=g) * 0.02
    for k, v in sd.items():
        if k.startswith("text_embed."):
            t[k] = v + torch.randn(v.shape, generator=g) * 0.01
    return t


def switch_bytes(sd, tensors, precision):
    """Bytes one base -> adapter switch reads (fp32 masters / replacement tensors, A, B) and writes (packed operands)."""
    elem = {"f32": 4, "f16x3": 4, "bf16": 2, "f16": 2, "f16p": 2}[precision]
    rd = wr = 0
    for k, v in tensors.items():
        if k.endswith(".lora_A.weight"):
            w = sd[k[: -len(".lora_A.weight")] + ".weight"]
            ldw = (w.shape[1] + 63) // 64 * 64
            rd += 4 * (w.numel() + v.numel() + tensors[k.replace("lora_A", "lora_B")].numel())
            wr += w.shape[0] * ldw * (elem + (4 if precision == "f16p" and k.startswith("input_embed.") else 0))
        elif ".lora_" not in k:
            rd += 4 * v.numel()
            wr += 4 * v.numel()
    return rd, wr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="f16p")
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    arch = P.config.F5TTS_BASE
    nv = P.config.VOCAB_SIZE + 1
    sd = P.weights.synthetic_state_dict(P.weights.dit_param_shapes(arch, nv))
    tensors = recipe_adapter(sd, arch["depth"])
    tr = P.DiT(**arch, text_num_embeds=nv, mel_dim=100, precision=args.precision)
    tr.load_state_dict(sd)
    tr.add_adapter("ft", tensors, **RECIPE)
    tr.to("cuda:0")
    tr.engine()
    torch.cuda.synchronize()
    for name in ("ft", None):   # untimed: first touch
        tr.set_adapter(name)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    for i in range(args.reps):
        tr.set_adapter("ft" if i % 2 == 0 else None)
    b.record()
    host_us = (time.perf_counter() - t0) / args.reps * 1e6
    b.synchronize()
    us = a.elapsed_time(b) * 1e3 / args.reps
    rd, wr = switch_bytes(sd, tensors, args.precision)
    print(f"{args.precision} f5_set_adapter: {us:.1f} us of device time per switch (HIP events over {args.reps} switches, base <-> adapter), "
          f"{host_us:.1f} us of host time per call; {rd / 1e6:.1f} MB read + {wr / 1e6:.1f} MB written = {(rd + wr) / us / 1e6:.2f} TB/s", flush=True)
    tr.set_adapter(None)
    # (2) the rebuild path
    merged = A.merge_adapter(sd, tensors, rule="matmul", **RECIPE)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tr2 = P.DiT(**arch, text_num_embeds=nv, mel_dim=100, precision=args.precision)
    tr2.load_state_dict(merged)
    tr2.to("cuda:0")
    tr2.engine()
    torch.cuda.synchronize()
    print(f"{args.precision} new engine from the host-merged state dict (load_state_dict + upload + f5_finalize): "
          f"{(time.perf_counter() - t0) * 1e3:.0f} ms of wall time (the host merge itself not counted)", flush=True)
    # (3) layernorm_kernel for scale
    lib = P.lib.load()
    R, D = 32768, 1024
    x = torch.randn(R, D, device="cuda:0")
    sc = torch.zeros(1, D, device="cuda:0")
    out = torch.empty_like(x)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for _ in range(5):
        P.lib.check(lib.f5k_layernorm_mod(C.c_void_p(x.data_ptr()), C.c_void_p(sc.data_ptr()), C.c_void_p(sc.data_ptr()),
                                          C.c_void_p(out.data_ptr()), R, D, R, 1e-6, st), "f5k_layernorm_mod")
    torch.cuda.synchronize()
    print(f"layernorm_kernel reference: 5 launches on f32 [{R}, {D}] ({R * D * 8 / 1e6:.1f} MB per launch): see the profiler's kernel stats")


if __name__ == "__main__":
    main()
