"""Cost of the held-out flow loss at F5-TTS Base size (synthetic weights, the reference recipe's adapters):

  (1) one f5_flow_loss call at one frame budget (f16p by default): device time by HIP events, beside one f5_dit_forward of the same
      batch -- the difference is the glue (flow_mix, flow_loss, flow_loss_finish and two small uploads);
  (2) infer.heldout_loss over K resident adapters on one engine, wall time, beside the only other way to rank K fine-tunes:
      K fresh engines, each from a host-merged state dict (load_state_dict + upload + f5_finalize + the same heldout_loss).

    python tools/flow_loss_time.py [--precision f16p] [--frames 38400] [--len 768] [--adapters 4] [--utts 16] [--times 8]
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f5_tts_amd as P  # noqa: E402
from adapter_switch_time import RECIPE, recipe_adapter  # noqa: E402
from f5_tts_amd import adapters as A  # noqa: E402


def build(sd, arch, nv, precision, adapters=None):
    tr = P.DiT(**arch, text_num_embeds=nv, mel_dim=100, precision=precision)
    tr.load_state_dict(sd)
    for name, t in (adapters or {}).items():
        tr.add_adapter(name, t, **RECIPE)
    model = P.CFM(transformer=tr, mel_spec_module=P.mel.MelSpec()).to("cuda:0")
    tr.engine()
    return model


def events(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="f16p")
    ap.add_argument("--frames", type=int, default=38400, help="frame budget of one batch")
    ap.add_argument("--len", type=int, default=768, help="frames per utterance")
    ap.add_argument("--adapters", type=int, default=4)
    ap.add_argument("--utts", type=int, default=16)
    ap.add_argument("--times", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    arch, nv = P.config.F5TTS_BASE, P.config.VOCAB_SIZE + 1
    sd = P.weights.synthetic_state_dict(P.weights.dit_param_shapes(arch, nv))
    tensors = {f"ft{i}": recipe_adapter(sd, arch["depth"], seed=1 + i) for i in range(args.adapters)}
    g = torch.Generator().manual_seed(0)

    # (1) one call at the frame budget
    model = build(sd, arch, nv, args.precision, tensors)
    eng = model.transformer.engine()
    B, N = max(1, args.frames // args.len), args.len
    x1, x0 = torch.randn(B, N, 100, generator=g).to("cuda:0"), torch.randn(B, N, 100, generator=g).to("cuda:0")
    text = torch.randint(0, nv - 1, (B, 64), generator=g)
    t, span, lens = [(b + 0.5) / B for b in range(B)], [(N // 8, N)] * B, [N] * B
    ms_loss = events(lambda: eng.flow_loss(x1, x0, text, t, span, lens=lens, want_pred=False, want_cond=False, want_frame_err=False), args.reps)
    ms_fwd = events(lambda: eng.forward(x0, x1, text, t, lens=lens), args.reps)
    print(f"{args.precision} B={B} N={N} ({B * N} frames): f5_flow_loss {ms_loss:.2f} ms per call, f5_dit_forward {ms_fwd:.2f} ms per call "
          f"(HIP events over {args.reps} calls, host staging of the arguments included in both)", flush=True)

    # (2) K adapters on one engine against K fresh engines
    mels = [torch.randn(args.len - 16 * (u % 8), 100, generator=g) for u in range(args.utts)]
    texts = [torch.randint(0, nv - 1, (48 + u % 16,), generator=g) for u in range(args.utts)]
    names = list(tensors)
    kw = dict(times=args.times, batch_frames=args.frames)
    P.infer.heldout_loss(model, mels, texts, adapters=names[:1], **kw)   # untimed: arena growth
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = P.infer.heldout_loss(model, mels, texts, adapters=names, **kw)
    wall_resident = time.perf_counter() - t0
    t0 = time.perf_counter()
    for name in names:
        merged = A.merge_adapter(sd, tensors[name], rule="contract", **RECIPE)
        fresh = build(merged, arch, nv, args.precision)
        P.infer.heldout_loss(fresh, mels, texts, **kw)
        del fresh
    wall_fresh = time.perf_counter() - t0
    rows = args.utts * args.times
    print(f"{args.precision} heldout_loss, {args.utts} utterances x {args.times} times = {rows} rows, {len(names)} adapters: one resident engine "
          f"{wall_resident * 1e3:.0f} ms of wall time, {len(names)} fresh engines on host-merged weights {wall_fresh * 1e3:.0f} ms "
          f"(losses {[round(res[n]['loss'], 5) for n in names]})", flush=True)


if __name__ == "__main__":
    main()
