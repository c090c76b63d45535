"""Float64 restatement of the MMDiT forward (the reference's backbones/mmdit.py:30-213, MMDiTBlock modules.py:743-771,
JointAttnProcessor modules.py:555-645), written from the formulas, with pieces of oracle/f5_oracle.py where the DiT shares them
(time features, conv position embedding, rotary embedding, final layer, the sample() argument handling and the ODE loop).

It gives the midpoint and precision tests a yardstick that does not travel from the reference: `forward` evaluates one backbone call
in float64 on the float32 weights and returns it in the dtype of `x`; `sample` is oracle.f5_oracle.sample (float32 ODE state and time
grid, as the reference keeps them) with that forward, under whichever solver tests/ode_oracle.py has installed.

The joint sequence is the reference's own order here (audio first, text second); the engine's text-first layout must not show.
"""
from __future__ import annotations

import contextlib

import torch
import torch.nn.functional as F

from oracle import f5_oracle as O

_W64: dict = {}


def _double(W):
    key = id(W)
    if key not in _W64 or _W64[key][0] is not W:
        _W64.clear()
        _W64[key] = (W, {k: v.double() for k, v in W.items()})
    return _W64[key][1]


def text_embed(W, cfg, text, drop_text=False):
    """mmdit.py:40-61: lookup (0 is the filler) + the sinus row of the token's position; with mask_padding the rows whose ORIGINAL
    token is the filler are zero, whatever drop_text then makes of the tokens."""
    ids = text + 1
    filler = ids == 0
    if drop_text:
        ids = torch.zeros_like(ids)
    E = W["text_embed.text_embed.weight"]
    pos = O.text_pos_table(E.shape[1], 1024)[torch.arange(text.shape[1]).clamp(max=1023)].to(E.dtype)
    e = E[ids] + pos
    if cfg.get("text_mask_padding", True):
        e = e.masked_fill(filler.unsqueeze(-1), 0.0)
    return e


def audio_embed(W, x, cond, drop_audio_cond=False):
    """mmdit.py:67-79: Linear(2 mel -> dim) on cat(x, cond), then the conv position embedding WITHOUT a mask, as a residual."""
    if drop_audio_cond:
        cond = torch.zeros_like(cond)
    h = O.linear(torch.cat((x, cond), dim=-1), W, "audio_embed.linear")
    return O.conv_pos_embed(W, "audio_embed.conv_pos_embed", h, None) + h


def _heads(t, H):
    b, n, _ = t.shape
    return t.view(b, n, H, -1).transpose(1, 2)


def joint_attention(W, cfg, pfx, x, c, mask, last):
    H, dh = cfg["heads"], cfg.get("dim_head", 64)
    n, nt = x.shape[1], c.shape[1]
    q, k, v = (_heads(O.linear(x, W, f"{pfx}.{m}"), H) for m in ("to_q", "to_k", "to_v"))
    cq, ck, cv = (_heads(O.linear(c, W, f"{pfx}.{m}"), H) for m in ("to_q_c", "to_k_c", "to_v_c"))
    if cfg.get("qk_norm") is not None:
        assert cfg["qk_norm"] == "rms_norm"
        q = F.rms_norm(q, (dh,), weight=W[pfx + ".q_norm.weight"], eps=1e-6)
        k = F.rms_norm(k, (dh,), weight=W[pfx + ".k_norm.weight"], eps=1e-6)
        cq = F.rms_norm(cq, (dh,), weight=W[pfx + ".c_q_norm.weight"], eps=1e-6)
        ck = F.rms_norm(ck, (dh,), weight=W[pfx + ".c_k_norm.weight"], eps=1e-6)
    fx, fc = O.rotary_freqs(n, dh).to(x.dtype), O.rotary_freqs(nt, dh).to(x.dtype)   # each stream from position 0, every head
    q, k, cq, ck = O.rotary_apply(q, fx), O.rotary_apply(k, fx), O.rotary_apply(cq, fc), O.rotary_apply(ck, fc)
    q, k, v = torch.cat((q, cq), dim=2), torch.cat((k, ck), dim=2), torch.cat((v, cv), dim=2)
    s = torch.matmul(q, k.transpose(-1, -2)) * (dh ** -0.5)
    if mask is not None:   # audio keys past an item's length; text keys never (padded text rows included)
        s = s.masked_fill(~F.pad(mask, (0, nt), value=True)[:, None, None, :], float("-inf"))
    o = torch.matmul(torch.softmax(s, dim=-1), v).transpose(1, 2).reshape(x.shape[0], n + nt, H * dh)
    ox = O.linear(o[:, :n], W, pfx + ".to_out.0")
    oc = None if last else O.linear(o[:, n:], W, pfx + ".to_out_c")
    if mask is not None:
        ox = ox.masked_fill(~mask.unsqueeze(-1), 0.0)
    return ox, oc


def _ln(x):
    return F.layer_norm(x, (x.shape[-1],), eps=1e-6)


def _ff(W, pfx, h):
    return O.linear(F.gelu(O.linear(h, W, pfx + ".ff.0.0"), approximate="tanh"), W, pfx + ".ff.2")


def block(W, cfg, i, x, c, t, mask):
    pfx = f"transformer_blocks.{i}"
    last = i == cfg["depth"] - 1
    st = F.silu(t)
    ex = O.linear(st, W, pfx + ".attn_norm_x.linear")
    x_shift, x_scale, x_gate, x_shift2, x_scale2, x_gate2 = (v[:, None] for v in torch.chunk(ex, 6, dim=1))
    ec = O.linear(st, W, pfx + ".attn_norm_c.linear")
    if last:   # AdaLayerNorm_Final: (scale, shift)
        c_scale, c_shift = (v[:, None] for v in torch.chunk(ec, 2, dim=1))
    else:
        c_shift, c_scale, c_gate, c_shift2, c_scale2, c_gate2 = (v[:, None] for v in torch.chunk(ec, 6, dim=1))
    ox, oc = joint_attention(W, cfg, pfx + ".attn", _ln(x) * (1 + x_scale) + x_shift, _ln(c) * (1 + c_scale) + c_shift, mask, last)
    if last:
        c = None
    else:
        c = c + c_gate * oc
        c = c + c_gate2 * _ff(W, pfx + ".ff_c", _ln(c) * (1 + c_scale2) + c_shift2)
    x = x + x_gate * ox
    x = x + x_gate2 * _ff(W, pfx + ".ff_x", _ln(x) * (1 + x_scale2) + x_shift2)
    return c, x


def forward(W, cfg, x, cond, text, time, mask=None, drop_audio_cond=False, drop_text=False, cfg_infer=False, cache=None, taps=None):
    """One MMDiT forward in float64 (weights, activations, softmax), returned in x's dtype.  `cache` is accepted and ignored (the
    text embedding is cheap); `taps`: a dict that receives the float64 intermediates under the fixture's names."""
    out_dtype = x.dtype
    W = _double(W)
    x, cond = x.double(), cond.double()
    time = time.reshape(-1) if time.ndim else time.repeat(x.shape[0])
    if time.shape[0] == 1 and x.shape[0] > 1:
        time = time.repeat(x.shape[0])
    h = O.sinus_features(time.float()).double()   # (the features are float32 arithmetic in the reference too)
    t = O.linear(F.silu(O.linear(h, W, "time_embed.time_mlp.0")), W, "time_embed.time_mlp.2")
    if cfg_infer:
        xs = torch.cat((audio_embed(W, x, cond, False), audio_embed(W, x, cond, True)), dim=0)
        c = torch.cat((text_embed(W, cfg, text, False), text_embed(W, cfg, text, True)), dim=0)
        t = torch.cat((t, t), dim=0)
        mask = torch.cat((mask, mask), dim=0) if mask is not None else None
    else:
        xs, c = audio_embed(W, x, cond, drop_audio_cond), text_embed(W, cfg, text, drop_text)
    if taps is not None:
        B = text.shape[0]
        taps["audio_embed"] = xs
        taps["text_cond"], taps["text_uncond"] = (c[:B], c[B:]) if cfg_infer else (c, None)
    for i in range(cfg["depth"]):
        c, xs = block(W, cfg, i, xs, c, t, mask)
        if taps is not None:
            taps[f"block{i}_x"] = xs
            if c is not None:
                taps[f"block{i}_c"] = c
    return O.final_layer(W, xs, t).to(out_dtype)


@contextlib.contextmanager
def _as_backbone():
    saved = O.dit_forward
    O.dit_forward = forward
    try:
        yield
    finally:
        O.dit_forward = saved


def sample(W, cfg, cond, text, duration, **kw):
    """cfm.py:83-229 with the MMDiT backbone: oracle.f5_oracle.sample's argument handling, mask rule, CFG and ODE loop (Euler, or
    whatever tests/ode_oracle.solver has installed) around `forward`."""
    with _as_backbone():
        return O.sample(W, cfg, cond, text, duration, backbone="DiT", **kw)
