"""GPU: the step glue of sample() -- the kernels csrc/engine_impl.h launches around every backbone evaluation -- each through the
launch helper the engine itself calls (f5k_pack_input, f5k_fill_rowmap, f5k_euler_cfg, f5k_midpoint_half_cfg, f5k_select_rows,
f5k_time_sinus, f5k_xrmsnorm, f5k_unett_assemble, f5k_cat2, f5k_strip_first_token), against tests/glue_oracle.py.

Copies and selections are held bit for bit; arithmetic to bounds from the number formats:
  Euler / midpoint half step   |err| <= 6 * 2^-24 * M, M = max|y| + |dt| (max|p| + |cfg| max|p - u|)   (glue_oracle.ode_bound)
  time features                |err| <= 4 x the largest error of torch's own f32 sin / cos on the same f32 arguments
  x_transformers RMSNorm       relative error <= 3e-6 per element (32-term lane sum, six shuffle steps, sqrt, divide, two multiplies:
                               about 47 * 2^-24); 16-bit rows = the f32 rows rounded; pre-split rows = split_planar64 of the plain ones
Every output is a Guarded buffer: what a launch must not touch keeps the sentinel (rows past *row_limit, everything past the last
row) or its prefill (the K-padding columns of the packed input rows), and the guard bands stay intact.  Inputs a kernel must not read
(prediction rows of alignment padding, everything past the last packed row) hold NaN."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import glue_oracle as G  # noqa: E402
from gpu_util import (DEV, ELEM_DTYPE, Guarded, k_cat2, k_euler_cfg, k_fill_rowmap, k_midpoint_half_cfg, k_pack_input,  # noqa: E402
                      k_select_rows, k_strip_first_token, k_time_sinus, k_unett_assemble, k_xrmsnorm, planar_planes, split_planar64)

EXTRA = 8   # rows of sentinel behind the last row a launch may write


def bits(t):
    """The bit pattern of a tensor, on the CPU (int32 for 4-byte elements, int16 for 2-byte ones)."""
    t = t.detach().contiguous().cpu()
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def ints(vals):
    return torch.tensor(vals, dtype=torch.int32, device=DEV)


def untouched(g, first_row):
    """Rows >= first_row of a 2-D Guarded still hold the sentinel, and so do the guard bands."""
    return bool((g.bits[first_row:] == g.sent).all()) and g.guards_intact()


def rand(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------------------------------------ fill_rowmap
def run_fill_rowmap(lens, halves):
    rs = G.row_start_table(lens, halves)
    rm = Guarded((rs[-1] + EXTRA, 2), torch.float32)
    return rs, k_fill_rowmap(ints(rs), rm, halves * len(lens))


def test_fill_rowmap_every_row_of_every_segment():
    """Up to 6 segments; spans of 4 rows and of more than 256 rows (more than one pass of the block)."""
    seen = set()
    for lens, halves in (([1, 300, 8], 2), ([4, 260, 5], 1), ([7], 1), ([5, 1, 8], 2)):
        rs, rm = run_fill_rowmap(lens, halves)
        seen |= {rs[i + 1] - rs[i] for i in range(len(rs) - 1)}
        assert len(rs) - 1 <= 6
        assert torch.equal(rm.bits[:rs[-1]].cpu(), G.rowmap_table(rs)), (lens, halves)
        assert untouched(rm, rs[-1]), "written past row_start[Bp]"
    assert 4 in seen and max(seen) > 256


# ------------------------------------------------------------------------------------------------- pack_input
PACK_FORMS = {"cfg": (2, 0), "cond_only": (1, 0), "cond_dropped": (1, 1)}   # form -> (halves, drop_cond_first)


def pack_inputs(B, N, mel, Dt, seed=0, exact=False):
    make = (lambda s, i: G.pattern(s, seed + i)) if exact else (lambda s, i: rand(s, seed + i))
    return make((B, N, mel), 1), make((B, N, mel), 2), make((B, N, Dt), 3), make((B, N, Dt), 4)   # x, cond, text_c, text_u


def run_pack_input(prec, form, B, N, mel, Dt, lens=None, exact=False):
    """Returns (the Guarded rows, the oracle's rows as f32, rows the launch may write, kin)."""
    halves, drop = PACK_FORMS[form]
    Bp, kin = halves * B, 2 * mel + Dt
    ldo = G.round_up(kin, 64)
    x, cond, tc, tu = pack_inputs(B, N, mel, Dt, exact=exact)
    ref = G.pack_input(x, cond, tc, tu, Bp, bool(drop))
    tables = {}
    if lens is None:
        live = Bp * N
        ref = ref.reshape(live, kin)
    else:
        rs, rm = run_fill_rowmap(lens, halves)   # the tables as the engine makes them: fill_rowmap itself, row_limit on the device
        rs_dev = ints(rs)
        live = rs[-1]
        ref = G.pack_rows(ref, rs, lens)
        tables = dict(rowmap=rm, row_limit=rs_dev[Bp:Bp + 1], lens=ints(lens))
    out = Guarded((live + EXTRA, ldo), ELEM_DTYPE[prec])
    out.bits[:live, kin:] = 0               # the K padding holds zero (the arena rule) and must keep it
    k_pack_input(prec, x.to(DEV), cond.to(DEV), tc.to(DEV), tu.to(DEV), out, Bp, drop, **tables)
    return out, ref, live, kin


@pytest.mark.parametrize("form", list(PACK_FORMS))
@pytest.mark.parametrize("mel,Dt", [(100, 512), (8, 4)])
@pytest.mark.parametrize("prec", ["f32", "bf16", "f16"])
def test_pack_input_padded_and_packed(prec, mel, Dt, form):
    for B, N, lens in ((2, 5, None), (3, 8, [5, 1, 8])):
        out, ref, live, kin = run_pack_input(prec, form, B, N, mel, Dt, lens)
        what = (prec, mel, Dt, form, lens)
        assert torch.equal(bits(out.value[:live, :kin]), bits(ref.to(out.dtype))), what
        assert not out.bits[:live, kin:].any(), f"{what}: the K-padding columns were written"
        assert untouched(out, live), f"{what}: a row >= *row_limit (or a guard band) was written"
        if lens is not None:
            halves = PACK_FORMS[form][0]
            rs = G.row_start_table(lens, halves)
            pad = [r for bp in range(halves * B) for r in range(rs[bp] + lens[bp % B], rs[bp + 1])]
            assert pad and not out.bits[pad, :kin].any(), f"{what}: alignment rows must be zero"


# ------------------------------------------------------------------------------------------------- ODE updates
def run_ode(kind, B, N, mel, cfg, use_cfg, lens=None, with_slot=True, exact=False, step=3):
    """One update.  Returns (y after: Guarded or the input tensor, the second output: Guarded or None, float64 reference, bound, y0, keep)."""
    halves = 2 if use_cfg else 1
    make = (lambda s, i: G.pattern(s, i)) if exact else (lambda s, i: rand(s, i))
    y0 = make((B, N, mel), 11)
    tgrid = G.sway_grid(8)
    keep = None
    if lens is None:
        pred = make((halves, B, N, mel), 12)
        p, u = pred[0], pred[1] if use_cfg else None
        pred_dev, tables = pred.to(DEV), {}
    else:
        rs = G.row_start_table(lens, halves)
        vals = make((rs[-1], mel), 12)
        rows = torch.full((rs[-1] + EXTRA, mel), float("nan"))   # alignment rows and everything past the last row: NaN, never to be read
        for bp in range(halves * B):
            n = lens[bp % B]
            rows[rs[bp]:rs[bp] + n] = vals[rs[bp]:rs[bp] + n]
        p = G.unpack_rows(rows, rs, lens, 0, B, N)
        u = G.unpack_rows(rows, rs, lens, 1, B, N) if use_cfg else None
        keep = G.frame_mask(lens, N)
        pred_dev, tables = rows.to(DEV), dict(row_start=ints(rs), lens=ints(lens))
    step_fn = G.euler_step if kind == "euler" else G.midpoint_half_step
    ref = step_fn(y0, p, u, tgrid, step, cfg, keep)
    bound = G.ode_bound(y0, p, u, tgrid, step, cfg)
    if kind == "euler":
        y = Guarded.like(y0.to(DEV))
        slot = Guarded(y0.shape, torch.float32) if with_slot else None
        k_euler_cfg(y, pred_dev, tgrid.to(DEV), step, cfg, use_cfg, slot, **tables)
        return y, slot, ref, bound, y0, keep
    y_mid = Guarded(y0.shape, torch.float32)
    y_dev = y0.to(DEV)
    k_midpoint_half_cfg(y_dev, pred_dev, tgrid.to(DEV), step, cfg, use_cfg, y_mid, **tables)
    return y_dev, y_mid, ref, bound, y0, keep


def check_ode(kind, res, what):
    y, second, ref, bound, y0, keep = res
    new = second if kind == "midpoint" else y   # the buffer that receives the step
    got = new.value.cpu()
    err = float((got.double() - ref).abs().max())
    print(f"[{what}] max |err| {err:.3e}  bound {bound:.3e}")
    assert err <= bound, f"{what}: {err:.3e} > {bound:.3e}"
    assert new.guards_intact()
    if keep is not None:   # frames past a length keep y bit for bit, in the state and in the second output
        frozen = ~keep.expand_as(y0)
        assert frozen.any() and torch.equal(bits(got)[frozen], bits(y0)[frozen]), f"{what}: a frame past its length moved"
    if kind == "euler" and second is not None:
        assert torch.equal(second.bits, y.bits) and second.guards_intact(), f"{what}: the trajectory slot is not the new state"
    if kind == "midpoint":
        assert torch.equal(bits(y), bits(y0)), f"{what}: the half step must not write y"


@pytest.mark.parametrize("cfg,use_cfg", [(2.0, 1), (0.0, 0)])
@pytest.mark.parametrize("mel", [100, 8])
@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("kind,with_slot", [("euler", True), ("euler", False), ("midpoint", True)])   # (y_mid is the half step's only output)
def test_ode_update_within_the_f32_bound(kind, with_slot, packed, mel, cfg, use_cfg):
    lens = G.PACKED["lens"] if packed else None
    res = run_ode(kind, G.PACKED["B"], G.PACKED["N"], mel, cfg, use_cfg, lens, with_slot)
    check_ode(kind, res, f"{kind} {'packed' if packed else 'plain'} mel {mel} cfg {cfg} slot {with_slot}")


# ------------------------------------------------------------------------------------------------ select_rows
def run_select_rows(rows, C, alias, exact=False):
    make = (lambda s, i: G.pattern(s, i)) if exact else (lambda s, i: rand(s, i))
    a, b = make((rows, C), 21), make((rows, C), 22)
    mask = (torch.arange(rows) * 7 % 3 == 0).to(torch.uint8)
    if alias:   # out = where(mask, cond, y) written over y
        out = Guarded.like(b.to(DEV))
        k_select_rows(a.to(DEV), out, mask.to(DEV), out)
        return out, G.select_rows(a, b, mask)
    out = Guarded((rows, C), torch.float32)
    k_select_rows(a.to(DEV), None, mask.to(DEV), out)
    return out, G.select_rows(a, None, mask)


@pytest.mark.parametrize("alias", [False, True])
def test_select_rows_is_bit_exact(alias):
    out, ref = run_select_rows(7, 100, alias)
    assert torch.equal(bits(out.value), bits(ref)) and out.guards_intact()


# ------------------------------------------------------------------------------------------------- time_sinus
def time_points():
    tg = G.sway_grid(8)
    return torch.tensor([0.0, 1.0, float(tg[3]), float(tg[5]), 0.5], dtype=torch.float32)   # 0, 1, two interior sway values, 0.5


def run_time_sinus():
    t = time_points()
    feat = Guarded((t.numel(), 256), torch.float32)
    return k_time_sinus(t.to(DEV), G.time_freqs().to(DEV), feat), t


def test_time_sinus_layout_and_accuracy():
    feat, t = run_time_sinus()
    assert t.numel() == 5 and t[0] == 0 and t[1] == 1 and 0 < t[2] < 1
    freq = G.time_freqs()
    ref = G.time_sinus(t, freq)                      # [S, 256]: sin half, then cos half, float64 of the f32 arguments
    arg = G.time_args(t, freq)
    torch_err = float((torch.cat((arg.sin(), arg.cos()), dim=-1).double() - ref).abs().max())   # torch's own f32 sin / cos
    err = float((feat.value.cpu().double() - ref).abs().max())
    print(f"[time_sinus] max |err| {err:.3e}  torch f32 {torch_err:.3e}  bound {4 * torch_err:.3e}")
    assert torch_err > 0 and err <= 4 * torch_err
    assert feat.guards_intact()
    assert torch.equal(bits(feat.value[0, :128]), bits(torch.zeros(128))) and torch.equal(bits(feat.value[0, 128:]), bits(torch.ones(128)))


# --------------------------------------------------------------------------------------------------- xrmsnorm
def xrms_inputs(D):
    x, g = rand((G.XRMS_ROWS, D), 31 + D), rand((D,), 32 + D)
    x[3] = 0          # an all-zero row: zeros, not NaN
    x[5] *= 1e-3      # rows of different scale
    x[6] *= 300.0
    return x, g


def run_xrmsnorm(prec, D, planar=0):
    x, g = xrms_inputs(D)
    out = Guarded((G.XRMS_ROWS, D), ELEM_DTYPE[prec])
    return k_xrmsnorm(prec, x.to(DEV), g.to(DEV), out, planar), x, g


@pytest.mark.parametrize("D", G.XRMS_DIMS)
def test_xrmsnorm_against_float64(D):
    out, x, g = run_xrmsnorm("f32", D)
    got, ref = out.value.cpu(), G.xrmsnorm(x, g)
    assert not got[3].any() and not torch.isnan(got).any(), "the all-zero row must give zeros"
    rel = ((got.double() - ref).abs() / ref.abs().clamp_min(1e-300))[ref != 0]
    print(f"[xrmsnorm D {D}] max relative error {float(rel.max()):.3e}  bound 3e-6")
    assert float(rel.max()) <= 3e-6 and torch.equal(got[ref == 0], torch.zeros_like(got[ref == 0]))
    assert out.guards_intact()
    for prec in ("bf16", "f16"):
        o16, _, _ = run_xrmsnorm(prec, D)
        assert torch.equal(bits(o16.value), bits(got.to(o16.dtype))), f"{prec}: not the f32 rows rounded"
        assert o16.guards_intact()
    if D % 32 == 0:
        pl, _, _ = run_xrmsnorm("f16x3", D, planar=1)
        assert torch.equal(pl.bits, split_planar64(out.value)) and pl.guards_intact(), "pre-split rows differ from the split of the plain rows"
        hi, lo = planar_planes(pl.bits)
        assert float((hi.float() + lo.float() - out.value).abs().max()) <= 2.0 ** -21 * float(out.value.abs().max())


# ------------------------------------------------------------------------------------------------- UNetT glue
def run_unett_assemble(Bp, N, D, stride, exact=False):
    make = (lambda s, i: G.pattern(s, i)) if exact else (lambda s, i: rand(s, i))
    h, temb = make((Bp, N, D), 41), make((Bp, D), 42)
    x = Guarded((Bp, N + 1, D), torch.float32)
    return k_unett_assemble(h.to(DEV), temb.to(DEV), stride, x), G.unett_assemble(h, temb, stride)


@pytest.mark.parametrize("stride", [0, 64])
def test_unett_assemble_is_bit_exact(stride):
    x, ref = run_unett_assemble(3, 5, 64, stride)
    assert torch.equal(bits(x.value), bits(ref)) and x.guards_intact()


def run_cat2(prec, rows, D, planar=0, exact=False):
    make = (lambda s, i: G.pattern(s, i)) if exact else (lambda s, i: rand(s, i))
    x, skip = make((rows, D), 51), make((rows, D), 52)
    out = Guarded((rows, 2 * D), ELEM_DTYPE[prec])
    return k_cat2(prec, x.to(DEV), skip.to(DEV), out, planar), G.cat2(x, skip)


@pytest.mark.parametrize("prec", ["f32", "bf16", "f16"])
def test_cat2_is_bit_exact(prec):
    out, ref = run_cat2(prec, 9, 64)
    assert torch.equal(bits(out.value), bits(ref.to(out.dtype))) and out.guards_intact()


def test_cat2_planar_is_the_split_of_the_plain_rows():
    out, ref = run_cat2("f16x3", 9, 64, planar=1)
    assert torch.equal(out.bits, split_planar64(ref.to(DEV))) and out.guards_intact()
    hi, lo = planar_planes(out.bits)
    assert float((hi.float() + lo.float() - ref.to(DEV)).abs().max()) <= 2.0 ** -21 * float(ref.abs().max())


def run_strip(Bp, N, C, exact=False):
    inp = G.pattern((Bp, N + 1, C), 61) if exact else rand((Bp, N + 1, C), 61)
    out = Guarded((Bp, N, C), torch.float32)
    return k_strip_first_token(inp.to(DEV), out), G.strip_first_token(inp)


def test_strip_first_token_is_bit_exact():
    out, ref = run_strip(3, 5, 100)
    assert torch.equal(bits(out.value), bits(ref)) and out.guards_intact()


# ------------------------------------------------------------------------------- the grid-stride loops' second pass
# (ew_blocks caps a launch at 4096 x 256 work items; tests/test_step_glue.py checks that each of these shapes has more)
def test_strided_pack_input():
    c = G.STRIDED["pack_input"]
    out, ref, live, kin = run_pack_input("f32", "cfg", c["B"], c["N"], c["mel"], c["Dt"], exact=True)
    assert torch.equal(bits(out.value[:live, :kin]), bits(ref)) and not out.bits[:live, kin:].any() and untouched(out, live)


@pytest.mark.parametrize("name", ["euler", "euler_packed", "midpoint", "midpoint_packed"])
def test_strided_ode_update(name):
    c = G.STRIDED[name]
    kind = name.split("_")[0]
    check_ode(kind, run_ode(kind, c["B"], c["N"], c["mel"], 2.0, 1, c.get("lens"), exact=True), f"strided {name}")


def test_strided_copies():
    c = G.STRIDED["select_rows"]
    for alias in (False, True):
        out, ref = run_select_rows(c["rows"], c["C"], alias, exact=True)
        assert torch.equal(bits(out.value), bits(ref)) and out.guards_intact()
    c = G.STRIDED["unett_assemble"]
    out, ref = run_unett_assemble(c["Bp"], c["N"], c["D"], c["D"], exact=True)
    assert torch.equal(bits(out.value), bits(ref)) and out.guards_intact()
    c = G.STRIDED["cat2"]
    out, ref = run_cat2("f32", c["rows"], c["D"], exact=True)
    assert torch.equal(bits(out.value), bits(ref)) and out.guards_intact()
    c = G.STRIDED["strip_first_token"]
    out, ref = run_strip(c["Bp"], c["N"], c["C"], exact=True)
    assert torch.equal(bits(out.value), bits(ref)) and out.guards_intact()


# ------------------------------------------------------------------------------------------------ determinism
def every_glue_kernel_once():
    """The output bits of one launch of every glue kernel, in each of its forms."""
    p = G.PACKED
    outs = [run_fill_rowmap([1, 300, 8], 2)[1].bits]
    for prec in ("f32", "bf16", "f16"):
        outs += [run_pack_input(prec, "cfg", 2, 5, 100, 512)[0].bits, run_pack_input(prec, "cfg", 3, 8, 100, 512, [5, 1, 8])[0].bits,
                 run_xrmsnorm(prec, 68)[0].bits, run_cat2(prec, 9, 64)[0].bits]
    for lens in (None, p["lens"]):
        y, slot = run_ode("euler", p["B"], p["N"], 100, 2.0, 1, lens)[:2]
        outs += [y.bits, slot.bits, run_ode("midpoint", p["B"], p["N"], 100, 2.0, 1, lens)[1].bits]
    outs += [run_select_rows(7, 100, False)[0].bits, run_select_rows(7, 100, True)[0].bits, run_time_sinus()[0].bits,
             run_xrmsnorm("f16x3", 1024, planar=1)[0].bits, run_unett_assemble(3, 5, 64, 0)[0].bits, run_cat2("f16x3", 9, 64, planar=1)[0].bits,
             run_strip(3, 5, 100)[0].bits]
    return [o.clone() for o in outs]


def test_every_glue_kernel_is_deterministic():
    first, second = every_glue_kernel_once(), every_glue_kernel_once()
    assert len(first) == len(second) >= 20
    for i, (a, b) in enumerate(zip(first, second)):
        assert torch.equal(a, b), f"output {i} differs between two runs"
