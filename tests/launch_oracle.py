"""float64 references of attention and the conv position embedding for the forms the engine launches them in: every batch row
is computed ON ITS OWN -- over its first `len` keys / queries / tokens, as if no other row and no padding existed -- so that a
kernel that lets a neighbour, a pad row or a stale column in can not agree with it.  Plain torch, runs on any device; checked
against the masked whole-batch formulations in tests/test_launch_forms.py."""
import torch
import torch.nn.functional as F

TDTYPE = {"bf16": torch.bfloat16, "f16": torch.float16}
L2E = 1.4426950408889634


def rnd(prec, x):
    """x as a 16-bit MFMA operand type sees it (f32 / f16x3: unchanged -- the hi + lo f16 halves carry 22 bits)."""
    return x if prec in ("f32", "f16x3") else x.to(TDTYPE[prec]).float()


def as_operands(mode, q, k, v):
    """What an attention path multiplies, as f32 tensors of unscaled q, k, v:
      bf16 / f16 / attn16 (the f16 kernel under f16x3): k, v and q * attention_q_scale (dim_head^-0.5 * log2 e, attn2.h) rounded to
        the operand type;
      f16x3/hiN (the split kernel, hi_only = N): bit 0 rounds q * 0.125 and k to f16 (K Q^T as the plain f16 product), bit 1 rounds
        v to f16 (V^T P^T likewise);
      f32, f16x3: nothing is rounded."""
    if mode in ("f32", "f16x3"):
        return q, k, v
    if mode.startswith("f16x3/hi"):
        hi = int(mode[-1])
        if hi & 1:
            q, k = rnd("f16", q * 0.125) / 0.125, rnd("f16", k)
        return q, k, rnd("f16", v) if hi & 2 else v
    prec = "f16" if mode == "attn16" else mode
    qs = 0.125 * L2E
    return rnd(prec, q * qs) / qs, rnd(prec, k), rnd(prec, v)


def row_start(lens, halves=2):
    """The engine's RowPack table of `halves` x len(lens) batch rows (both CFG halves read lens[b % B]): every span is the row's
    length rounded up to a multiple of 4, the last entry is the total row count."""
    rs = [0]
    for b in range(halves * len(lens)):
        rs.append(rs[-1] + (lens[b % len(lens)] + 3) // 4 * 4)
    return rs


def attention_alone(q, k, v, kv_lens=None, q_lens=None):
    """q, k, v [Bp, H, N, 64] (unscaled q) -> a list of Bp float64 tensors [q_len_b, H * 64]: softmax(q k^T / 8) v of batch row b over
    its first kv_len_b keys and q_len_b queries; the tables are indexed b % len(table), None = N."""
    Bp, H, N, _ = q.shape
    out = []
    for b in range(Bp):
        nk = N if kv_lens is None else min(N, kv_lens[b % len(kv_lens)])
        nq = N if q_lens is None else min(N, q_lens[b % len(q_lens)])
        qb, kb, vb = q[b, :, :nq].double(), k[b, :, :nk].double(), v[b, :, :nk].double()
        o = torch.softmax(qb @ kb.transpose(-1, -2) / 8.0, dim=-1) @ vb      # [H, nq, 64]
        out.append(o.transpose(0, 1).reshape(nq, H * 64))
    return out


def convpos_alone(prec, x, w, bias, res=None):
    """One utterance alone: x [len, D] (its valid rows only), w [D, D / 16, 31], res [len, D] or None -> float64 [len, D] =
    mish(conv1d(x, zero padding 15 at ITS OWN ends, 16 groups) + bias) + res, with x and w as the operand type of prec holds them."""
    h = F.conv1d(rnd(prec, x).double().t()[None], rnd(prec, w).double(), bias.double(), padding=15, groups=16)
    y = F.mish(h)[0].t()
    return y if res is None else y + res.double()
