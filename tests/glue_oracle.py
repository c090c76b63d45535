"""Plain-torch restatements of the step glue of sample() (csrc/elementwise.h): what every kernel around a backbone evaluation must write,
index for index, in float64 where arithmetic is involved.  tests/test_step_glue.py ties each restatement to an independent
formulation on the CPU; tests/test_step_glue_gpu.py holds the kernels to them.

Shapes follow the engine: B utterances of N frames, Bp = B or 2 B batch rows (rows b' >= B are the unconditional half of a CFG forward),
`halves` = Bp / B.  A packed batch (RowPack) gives batch row b' the rows row_start[b'] .. row_start[b' + 1] - 1, its length rounded up to
4; the positions past the length inside that span are the alignment rows."""
import math

import torch

EW_CAP_ITEMS = 4096 * 256   # ew_blocks: a launch has at most 4096 blocks of 256 threads; work items past that take the loop's next pass
EPS32 = 2.0 ** -24          # half an ulp of 1.0 in f32: the relative error of one rounding


def round_up(v, a):
    return (v + a - 1) // a * a


# ------------------------------------------------------------------------------------------------ row tables
def row_start_table(lens, halves):
    """upload_small's table: halves * B spans of round_up(len, 4) rows, from 0."""
    rs = [0]
    for q in range(halves * len(lens)):
        rs.append(rs[-1] + round_up(lens[q % len(lens)], 4))
    return rs


def rowmap_table(row_start):
    """fill_rowmap: row r of segment b' is (b', r - row_start[b']).  int32 [row_start[-1], 2]."""
    pairs = [(b, n) for b in range(len(row_start) - 1) for n in range(row_start[b + 1] - row_start[b])]
    return torch.tensor(pairs, dtype=torch.int32).reshape(-1, 2)


# -------------------------------------------------------------------------------------------- input packing
def pack_input(x, cond, text_c, text_u, Bp, drop_cond_first=False):
    """[Bp, N, 2 mel + Dt]: rows b' < B are [x | cond (0 when dropped) | text_c], rows b' >= B are [x | 0 | text_u]."""
    B = x.shape[0]
    zero = torch.zeros_like(cond)
    first = torch.cat((x, zero if drop_cond_first else cond, text_c), dim=-1)
    if Bp == B:
        return first
    assert Bp == 2 * B
    return torch.cat((first, torch.cat((x, zero, text_u), dim=-1)), dim=0)


def pack_rows(padded, row_start, lens):
    """The packed rows of a padded [Bp, N, K]: [row_start[-1], K]; alignment rows (position >= the sample's length) are zero."""
    Bp, N, K = padded.shape
    out = torch.zeros(row_start[-1], K, dtype=padded.dtype)
    for bp in range(Bp):
        n = lens[bp % len(lens)]
        out[row_start[bp]:row_start[bp] + n] = padded[bp, :n]
    return out


def unpack_rows(rows, row_start, lens, half, B, N, fill=0.0):
    """The reverse reading the ODE updates make: [B, N, C] with frame n < lens[b] of utterance b from row row_start[half * B + b] + n."""
    out = torch.full((B, N, rows.shape[-1]), fill, dtype=rows.dtype)
    for b in range(B):
        r0 = row_start[half * B + b]
        out[b, :lens[b]] = rows[r0:r0 + lens[b]]
    return out


def frame_mask(lens, N):
    """[B, N, 1] bool: frame n of utterance b lies inside its length."""
    return (torch.arange(N)[None, :] < torch.tensor(lens)[:, None])[..., None]


# ------------------------------------------------------------------------------------------------ ODE updates
def sway_grid(steps, coef=-1.0):
    """cfm.py's time grid, f32: t = linspace(0, 1, steps + 1); t + coef * (cos(pi / 2 t) - 1 + t) -- non-uniform for coef != 0."""
    t = torch.linspace(0, 1, steps + 1, dtype=torch.float32)
    return t + coef * (torch.cos(torch.pi / 2 * t) - 1 + t)


def dt_f32(tgrid, step):
    """The step as the kernels form it: the f32 difference of two f32 grid points."""
    assert tgrid.dtype == torch.float32
    return (tgrid[step + 1] - tgrid[step]).double()


def velocity(p, u, cfg):
    """p + (p - u) * cfg in float64 (cfm.py:190-191); u None: no CFG."""
    p = p.double()
    return p if u is None else p + (p - u.double()) * cfg


def euler_step(y, p, u, tgrid, step, cfg, keep=None):
    """y + dt * v in float64; where `keep` ([B, N, 1] bool, the frames inside a length) is False the state keeps y."""
    new = y.double() + dt_f32(tgrid, step) * velocity(p, u, cfg)
    return new if keep is None else torch.where(keep, new, y.double())


def midpoint_half_step(y, p, u, tgrid, step, cfg, keep=None):
    """y + v * (dt / 2) in float64 (torchdiffeq Midpoint._step_func's y_mid)."""
    new = y.double() + velocity(p, u, cfg) * (0.5 * dt_f32(tgrid, step))
    return new if keep is None else torch.where(keep, new, y.double())


def ode_bound(y, p, u, tgrid, step, cfg):
    """6 * 2^-24 * M with M = max|y| + |dt| (max|p| + |cfg| max|p - u|): five f32 roundings of partial results no larger than M (the
    difference, its product with cfg, the sum with p, the product with dt, the sum with y), each 2^-24 relative, and their growth."""
    dt = abs(float(dt_f32(tgrid, step)))
    spread = 0.0 if u is None else abs(cfg) * float((p.double() - u.double()).abs().max())
    return 6 * EPS32 * (float(y.abs().max()) + dt * (float(p.abs().max()) + spread))


# ----------------------------------------------------------------------------------------------- small kernels
def select_rows(a, b, rowmask):
    """where(rowmask, a, b) row-wise; b None reads as zeros."""
    return torch.where(rowmask.bool()[:, None], a, torch.zeros_like(a) if b is None else b)


def time_freqs():
    """modules.py:157-164: exp(arange(128) * -log(10000) / 127), f32 (aux.time_freqs)."""
    return torch.exp(torch.arange(128).float() * -(math.log(10000) / 127))


def time_args(t, freq):
    """The arguments as the kernel forms them, in f32: (1000 t[s]) * freq[j].  [S, 128]"""
    assert t.dtype == freq.dtype == torch.float32
    return (1000.0 * t)[:, None] * freq[None, :]


def time_sinus(t, freq):
    """[S, 256] float64: the sin half, then the cos half, of the f32 arguments."""
    arg = time_args(t, freq).double()
    return torch.cat((arg.sin(), arg.cos()), dim=-1)


def xrmsnorm(x, g):
    """x_transformers RMSNorm in float64: x / max(|x|_2, 1e-12) * sqrt(D) * g (an all-zero row gives zeros)."""
    x = x.double()
    nrm = x.pow(2).sum(-1, keepdim=True).sqrt().clamp_min(1e-12)
    return x / nrm * math.sqrt(x.shape[-1]) * g.double()


def unett_assemble(h, temb, temb_stride):
    """[Bp, N + 1, D]: the time token of batch row b' (temb_stride 0: one shared row) in front of its N frames."""
    Bp, N, D = h.shape
    t = torch.stack([temb.reshape(-1)[b * temb_stride:b * temb_stride + D] for b in range(Bp)])
    return torch.cat((t[:, None, :], h), dim=1)


def cat2(x, skip):
    return torch.cat((x, skip), dim=-1)


def strip_first_token(x):
    return x[:, 1:, :].contiguous()


# ------------------------------------------------------------------------ the cases of tests/test_step_glue_gpu.py
# (tests/test_step_glue.py checks on the CPU that they reach what they are there for)
PACKED = dict(B=3, N=12, lens=[12, 5, 1])     # a full utterance, one with alignment rows (5 -> 8), and a single frame
XRMS_DIMS = (64, 68, 1024, 2048)              # 68: 17 lanes of 4 hold data, the other 47 lanes of the wave hold none
XRMS_ROWS = 9                                 # 4 rows per block: the third block is partial
# one case per grid-stride kernel whose float4 items exceed one pass of the capped grid; items = float4 work items of the launch
STRIDED = {
    "pack_input": dict(B=1, Bp=2, N=2946, mel=100, Dt=512),        # 5,892 rows x 178
    "euler": dict(B=3, N=14000, mel=100),
    "euler_packed": dict(B=3, N=14000, mel=100, lens=[14000, 13998, 1]),
    "midpoint": dict(B=3, N=14000, mel=100),
    "midpoint_packed": dict(B=3, N=14000, mel=100, lens=[14000, 13998, 1]),
    "select_rows": dict(rows=42000, C=100),
    "unett_assemble": dict(Bp=3, N=21846, D=64),
    "cat2": dict(rows=32769, D=64),
    "strip_first_token": dict(Bp=3, N=14000, C=100),
}


def strided_items(name):
    c = STRIDED[name]
    if name == "pack_input":
        return c["Bp"] * c["N"] * (2 * c["mel"] + c["Dt"]) // 4
    if name in ("euler", "euler_packed", "midpoint", "midpoint_packed"):
        return c["B"] * c["N"] * c["mel"] // 4
    if name == "select_rows":
        return c["rows"] * c["C"] // 4
    if name == "unett_assemble":
        return c["Bp"] * (c["N"] + 1) * c["D"] // 4
    if name == "cat2":
        return c["rows"] * 2 * c["D"] // 4
    return c["Bp"] * c["N"] * c["C"] // 4


def pattern(shape, seed, device="cpu"):
    """A cheap exact pattern: multiples of 1/8 in [-64, 64), no two neighbours alike."""
    n = 1
    for s in shape:
        n *= s
    i = torch.arange(n, device=device, dtype=torch.int64)
    return (((i * 7919 + seed * 104729) % 1024 - 512).float() / 8).reshape(shape)
