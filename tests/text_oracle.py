"""Test-side float64 reference of the text encoder: token ids -> text embedding [B, N, text_dim] for DiT and UNetT.

Written the obvious way for the tests of csrc/elementwise.h's text kernels: one sample at a time at its own length,
explicit boolean masks, torch.nn.functional ops on double tensors, the sinusoidal position table evaluated in float64
too.  It imports neither the engine nor oracle/f5_oracle.py; tests/test_text_encoder.py pins the two references
against each other.

What it computes (the published F5-TTS / E2-TTS text embedding):

    ids   = text + 1, cut or filled with the filler id 0 to the sample's length L
    h     = E[ids]                                   (drop_text: every id becomes 0 AFTER the padding mask is taken)
    with conv layers:
        h = h + pos[0:L]                             (UNetT: pos[min(n, 4095)])
        text_mask_padding: filler rows of h are zeroed, now and after every block
        block: h + pwconv2(GRN(gelu_erf(pwconv1(LayerNorm(dwconv7(h))))))
        GRN:   Gx[c] = ||x[:, c]||_2 over the L rows,  Nx = Gx / (mean_c Gx + 1e-6),  gamma * (x * Nx) + beta + x
    average upsampling (DiT option): the non-filler tokens are repeated to fill L rows, the LAST L % tl of them once
        more than the others; a sample without such a token stays zero
    DiT embeds sample b at L = lens[b] and leaves rows L..N-1 zero; UNetT always embeds at L = N.

`mutate` names ONE deliberate error (MUTATIONS).  Those exist to show that the tests' inputs can tell a wrong text
encoder from a right one (tests/test_text_encoder.py); nothing else may pass one.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

F64 = torch.float64

MUTATIONS = (
    "grn_norm_over_padded_n",     # GRN norm over the padded N rows instead of the sample's own L
    "grn_nx_times_1p05",          # Nx scaled by 1.05
    "grn_mean_over_text_dim",     # channel mean of Gx divides by text_dim instead of the 2 * text_dim channels
    "dw_taps_reversed",           # depthwise taps in reverse order
    "conv_reads_past_length",     # embedded at the padded length, then cut: the conv sees neighbours past L
    "filler_not_rezeroed",        # text_mask_padding: filler rows zeroed once before the blocks, not after each
    "pad_mask_after_drop_text",   # padding mask taken from the ids after drop_text
    "gelu_tanh",                  # tanh approximation in place of erf
    "pos_shifted_one_row",        # position row n + 1 for token n
    "unett_pos_not_clamped",      # UNetT position row n instead of min(n, 4095)
    "upsample_extra_to_first",    # average upsampling: the extra repeat goes to the first L % tl tokens
)


def pos_table64(dim: int, rows: int, first: int = 0) -> torch.Tensor:
    """[rows, dim] = [cos(n * f_j), sin(n * f_j)], f_j = 10000 ** (-2j / dim), n = first .. first + rows - 1."""
    freqs = 10000.0 ** (-torch.arange(0, dim, 2, dtype=F64)[: dim // 2] / dim)
    ang = torch.outer(torch.arange(first, first + rows, dtype=F64), freqs)
    return torch.cat([ang.cos(), ang.sin()], dim=-1)


def _grn(x, gamma, beta, rows, text_dim, mutate):
    """x [R, 2 * text_dim]; the norm runs over the first `rows` rows (all R unless a mutation pads x)."""
    gx = x[:rows].pow(2).sum(dim=0).sqrt()
    mean = gx.sum() / (text_dim if mutate == "grn_mean_over_text_dim" else gx.numel())
    nx = gx / (mean + 1e-6)
    if mutate == "grn_nx_times_1p05":
        nx = nx * 1.05
    return gamma * (x * nx) + beta + x


def _block(W, p, h, n_padded, mutate):
    """One ConvNeXt-V2 block on h [L, Dt]."""
    L, Dt = h.shape
    x = h
    if mutate == "grn_norm_over_padded_n":      # the block as it runs on the zero-padded batch row
        x = F.pad(h, (0, 0, 0, n_padded - L))
    wk = W[p + ".dwconv.weight"]
    if mutate == "dw_taps_reversed":
        wk = wk.flip(-1)
    y = F.conv1d(x.t().unsqueeze(0), wk, W[p + ".dwconv.bias"], padding=3, groups=Dt)[0].t()
    y = F.layer_norm(y, (Dt,), W[p + ".norm.weight"], W[p + ".norm.bias"], eps=1e-6)
    y = F.linear(y, W[p + ".pwconv1.weight"], W[p + ".pwconv1.bias"])
    y = F.gelu(y, approximate="tanh" if mutate == "gelu_tanh" else "none")
    y = _grn(y, W[p + ".grn.gamma"].reshape(-1), W[p + ".grn.beta"].reshape(-1), y.shape[0], Dt, mutate)
    y = F.linear(y, W[p + ".pwconv2.weight"], W[p + ".pwconv2.bias"])
    return h + y[:L]


def _average_upsample(h, valid, mutate):
    """h [L, Dt], valid bool[L]: the valid rows repeated to fill L rows."""
    L = h.shape[0]
    tokens = h[valid]
    tl = tokens.shape[0]
    out = torch.zeros_like(h)
    if tl == 0:
        return out
    base, rem = L // tl, L % tl
    row = 0
    for j in range(tl):
        extra = j < rem if mutate == "upsample_extra_to_first" else j >= tl - rem
        reps = base + (1 if extra else 0)
        out[row:row + reps] = tokens[j]
        row += reps
    assert row == L
    return out


def _embed_one(W, arch, backbone, ids_in, L, n_padded, drop_text, mutate):
    """ids_in: i64[nt] of one sample (-1 = filler) -> f64[L, Dt]."""
    nt = ids_in.shape[0]
    ids = torch.zeros(L, dtype=torch.long)
    m = min(nt, L)
    ids[:m] = ids_in[:m] + 1
    pad = ids == 0
    if drop_text:
        ids = torch.zeros_like(ids)
        if mutate == "pad_mask_after_drop_text":
            pad = ids == 0
    h = W["text_embed.text_embed.weight"][ids]
    layers = arch.get("conv_layers", 0)
    mask_padding = arch.get("text_mask_padding", True)
    if layers > 0:
        Dt = h.shape[1]
        first = 1 if mutate == "pos_shifted_one_row" else 0
        if backbone == "UNetT":
            n = torch.arange(first, first + L)
            if mutate != "unett_pos_not_clamped":
                n = n.clamp(max=4095)
            pos = pos_table64(Dt, int(n.max()) + 1)[n]
        else:
            pos = pos_table64(Dt, L, first)
        h = h + pos
        if mask_padding:
            h = h.masked_fill(pad[:, None], 0.0)
        for i in range(layers):
            h = _block(W, f"text_embed.text_blocks.{i}", h, n_padded, mutate)
            if mask_padding and mutate != "filler_not_rezeroed":
                h = h.masked_fill(pad[:, None], 0.0)
    return h, pad


def text_embed64(sd, arch, text, N, lens=None, drop_text=False, backbone="DiT", mutate=None):
    """sd: {name: tensor} with the reference's state-dict names; arch: the arch dict (text_dim is read off the embedding
    table); text i64[B, nt] padded with -1; lens: per-sample lengths or None -> f64[B, N, text_dim]."""
    assert mutate is None or mutate in MUTATIONS, mutate
    W = {k: v.to(F64) for k, v in sd.items() if k.startswith("text_embed.")}
    B = text.shape[0]
    Dt = W["text_embed.text_embed.weight"].shape[1]
    out = torch.zeros(B, N, Dt, dtype=F64)
    upsample = bool(arch.get("text_embedding_average_upsampling", False))
    if upsample:
        assert backbone == "DiT" and arch.get("text_mask_padding", True)
    for b in range(B):
        L = N if (lens is None or backbone == "UNetT") else int(lens[b])
        if mutate == "conv_reads_past_length":
            h, pad = _embed_one(W, arch, backbone, text[b], N, N, drop_text, None)
            h, pad = h[:L], pad[:L]
        else:
            h, pad = _embed_one(W, arch, backbone, text[b], L, N, drop_text, mutate)
        if upsample:
            h = _average_upsample(h, ~pad, mutate)
        out[b, :L] = h
    return out
