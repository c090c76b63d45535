"""The f8 arithmetic contract of include/f5_hip.h (F5_PREC_F8) restated in torch, on the CPU or any device:

  * the row quantiser: one power-of-two scale per row (an e8m0 byte b, value 2^(b - 127): the smallest power of two s with
    amax / s <= 448 over the row's K real elements, b = 127 for a zero row) and OCP e4m3fn codes of x / s, round to nearest even --
    torch.float8_e4m3fn after a clamp to +-448 (an unclamped 500 converts to NaN);
  * dit_block_f8: oracle.f5_oracle.dit_block with the header's rounding points emulated -- e4m3 fake-quant with those scales on the
    operands of QKV, out-projection, FF1 and FF2 (xn from the f32 value; attention output and FF hidden rounded to f16 first; weights
    per output channel from the f32 master) and f16 wherever F5_PREC_F16P rounds inside a block (q / k / v, the softmax weights).
    Patched in as tests/study_ln_behind_product.py patches its blocks:  with f8_blocks(): O.sample(...)
"""
import contextlib

import torch
import torch.nn.functional as F

from oracle import f5_oracle as O

E4M3_MAX = 448.0


def scale_bytes(x, K=None):
    """e8m0 byte per row of x [..., ld], over the first K columns (the rest is padding and does not count)."""
    a = x[..., :K].abs().amax(dim=-1)
    m, e = torch.frexp(a)                       # a = m 2^e, 0.5 <= m < 1; 448 = 0.875 * 2^9
    b = e - 9 + (m > 0.875).to(e.dtype) + 127
    b = torch.where(a == 0, torch.full_like(b, 127), b.clamp(min=1))
    return b.to(torch.uint8)


def scale_values(b):
    return torch.exp2(b.to(torch.float32) - 127.0)


def quantise_rows(x, K=None):
    """x [..., ld] -> (codes uint8 [..., K], scale bytes uint8 [...]) per the contract."""
    b = scale_bytes(x, K)
    y = (x[..., :K] / scale_values(b).to(x.dtype)[..., None]).clamp(-E4M3_MAX, E4M3_MAX)
    return y.to(torch.float8_e4m3fn).view(torch.uint8), b


def dequantise(codes, b):
    return codes.view(torch.float8_e4m3fn).float() * scale_values(b)[..., None]


def fake_quant(x):
    """x as the e4m3 kernels see it: quantised row by row (last dim) and dequantised, in x's own dtype (f32, or the float64 of
    tests/flow_oracle.py: codes times a power of two are exact in both)."""
    c, b = quantise_rows(x)
    return dequantise(c, b).to(x.dtype)


def e4m3_step(y):
    """spacing of the e4m3 grid at |y| <= 448 (y already divided by the scale): 2^(floor(log2 |y|) - 3), 2^-9 below 2^-6"""
    e = torch.floor(torch.log2(y.abs().clamp_min(2.0 ** -6)))
    return torch.exp2(e - 3)


h16 = lambda a: a.half().to(a.dtype)   # noqa: E731


def lin8(a, W, name):
    """fake-quantised operands, f32 accumulate, + bias"""
    return F.linear(fake_quant(a), fake_quant(W[name + ".weight"])) + W[name + ".bias"]


def attention_f8(W, cfg, pfx, h, mask, freqs):
    b, n, _ = h.shape
    H, dh = cfg["heads"], cfg.get("dim_head", 64)
    q, k, v = (lin8(h, W, pfx + nm).view(b, n, H, dh).transpose(1, 2) for nm in (".to_q", ".to_k", ".to_v"))
    if cfg.get("qk_norm") is not None:   # (the engine stores raw f16 q / k, then norms and rotates them in place)
        q = F.rms_norm(h16(q), (dh,), weight=W[pfx + ".q_norm.weight"], eps=1e-6)
        k = F.rms_norm(h16(k), (dh,), weight=W[pfx + ".k_norm.weight"], eps=1e-6)
    pn = cfg.get("pe_attn_head")
    if pn is None:
        q, k = O.rotary_apply(q, freqs), O.rotary_apply(k, freqs)
    else:
        q = torch.cat((O.rotary_apply(q[:, :pn], freqs), q[:, pn:]), dim=1)
        k = torch.cat((O.rotary_apply(k[:, :pn], freqs), k[:, pn:]), dim=1)
    q, k, v = h16(q * dh ** -0.5), h16(k), h16(v)
    s = torch.matmul(q, k.transpose(-1, -2))
    if cfg.get("attn_mask_enabled", False) and mask is not None:
        s = s.masked_fill(~mask[:, None, None, :], float("-inf"))
    o = torch.matmul(h16(torch.softmax(s, dim=-1)), v).transpose(1, 2).reshape(b, n, H * dh)
    o = lin8(h16(o), W, pfx + ".to_out.0")   # ao: f16 first, then the stand-alone quantiser
    if mask is not None:
        o = o.masked_fill(~mask.unsqueeze(-1), 0.0)
    return o


def dit_block_f8(W, cfg, i, x, t, mask, freqs):
    pfx = f"transformer_blocks.{i}"
    dim = x.shape[-1]
    emb = O.linear(F.silu(t), W, pfx + ".attn_norm.linear")
    shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp = torch.chunk(emb, 6, dim=1)
    h = F.layer_norm(x, (dim,), eps=1e-6) * (1 + scale_msa[:, None]) + shift_msa[:, None]   # quantised from f32 (lin8)
    x = x + gate_msa.unsqueeze(1) * attention_f8(W, cfg, pfx + ".attn", h, mask, freqs)
    h = F.layer_norm(x, (dim,), eps=1e-6) * (1 + scale_mlp[:, None]) + shift_mlp[:, None]
    h = h16(F.gelu(lin8(h, W, pfx + ".ff.ff.0.0"), approximate="tanh"))                        # ffh: f16 first
    h = lin8(h, W, pfx + ".ff.ff.2")
    return x + gate_mlp.unsqueeze(1) * h


@contextlib.contextmanager
def f8_blocks():
    orig = O.dit_block
    O.dit_block = dit_block_f8
    try:
        yield
    finally:
        O.dit_block = orig
