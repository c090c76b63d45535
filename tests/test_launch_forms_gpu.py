"""GPU: attention and the conv position embedding in the forms the DiT engine launches them (f5k_attention_ex / f5k_convpos_ex make
the launch_* calls of engine_impl.h's attend / embed_input): 2B batch rows on a length table of B entries, q_lens, packed
output rows (RowPack), the f16x3 output forms (pre-split f32 rows, the f16 kernel's Of, hi_only), the 4-stage conv weight ring.

Reference: launch_oracle -- every batch row alone in float64 on the operands as its path rounds them (tests/test_launch_forms.py
ties it to the masked whole-batch formulations).  Bounds: attention Linf within the tol_r column of test_kernels_gpu.ATTN_TOLS
(attn16 and f16x3/hi1..3 round no more than the f16 kernel: its 8e-4); conv-pos Linf within 5e-5 max(1, |ref|max).

What the engine never writes -- q / k rows and V^T columns past an item's length, V^T columns [N, Npad), x rows past the length --
holds finite bits by the arena rule (internal.h) and must not matter: every case runs once with zeros there and once with finite
garbage of mixed sign (magnitudes up to 8160, exact in bf16 and f16), and what the launch wrote must agree bit for bit.  NaN / Inf
are never put into an input: the arena rule excludes them, and 0 * NaN in the V^T P^T product is NaN by construction.
Every output is a Guarded buffer: rows the launch must not touch keep the sentinel, the guard bands stay intact."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import DEV, Guarded, k_attention_ex, k_convpos_ex, planar_planes, split_planar64  # noqa: E402
import launch_oracle as LO  # noqa: E402

EXTRA = 8   # rows of sentinel behind the last packed row


def garbage(shape, seed):
    """Finite values of mixed sign, m * 2^e with m in 1..255: exact in bf16 and f16, magnitudes 1/16 .. 8160."""
    g = torch.Generator().manual_seed(seed)
    m = torch.randint(1, 256, shape, generator=g).float()
    e = torch.randint(-4, 6, shape, generator=g).float()
    sign = torch.randint(0, 2, shape, generator=g).float() * 2 - 1
    return (sign * m * torch.exp2(e)).to(DEV)


# ------------------------------------------------------------------------------------------------------ attention
# mode -> (precision, entry-point mode, hi_only, Linf bound against float64 of the rounded operands)
AMODES = {"f32": ("f32", 0, 0, 3e-5), "bf16": ("bf16", 0, 0, 6e-3), "f16": ("f16", 0, 0, 8e-4), "f16x3": ("f16x3", 0, 0, 3e-5),
          "f16x3/hi1": ("f16x3", 0, 1, 8e-4), "f16x3/hi2": ("f16x3", 0, 2, 8e-4), "f16x3/hi3": ("f16x3", 0, 3, 8e-4),
          "attn16": ("f16x3", 1, 0, 8e-4)}
PACKED_SHAPES = [(3, 2, 200, [200, 37, 129]),    # Bp * H = 12: the plain block map
                 (2, 4, 256, [256, 70])]         # Bp * H = 16: the XCD-remapped block map (attn_block_map)


def attn_inputs(Bp, H, N, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(Bp, H, N, 64, generator=g).to(DEV) for _ in range(3)]


def with_tails(ts, lens, junk):
    """Copies of q / k / v [Bp, H, N, 64] whose rows past each batch row's length are zero (junk False) or garbage."""
    out = []
    for i, t in enumerate(ts):
        t = t.clone()
        fill = garbage(t.shape, 100 + i) if junk else torch.zeros_like(t)
        for b in range(t.shape[0]):
            n = lens[b % len(lens)]
            t[b, :, n:] = fill[b, :, n:]
        out.append(t)
    return out


def attn_launch(mode, qkv, out_rows, junk, o_planar=0, **tables):
    prec, m, hi, _ = AMODES[mode]
    H = qkv[0].shape[1]
    out = Guarded((out_rows, H * 64), LO.TDTYPE.get(prec, torch.float32))
    return k_attention_ex(prec, *qkv, out, mode=m, hi_only=hi, o_planar=o_planar, vt_pad_fill=-6144.0 if junk else 0.0, **tables)


def attn_values(mode, out):
    """The output rows as f32 (attn16: hi + lo of the pre-split rows)."""
    if mode == "attn16":
        hi, lo = planar_planes(out.bits)
        return hi.float() + lo.float()
    return out.value.float()


def attn_case(mode, qkv, lens_of_tails, out_rows, spans, **tables):
    """Both fills of one launch form.  spans: per batch row (first output row, rows the reference covers, rows the launch writes).
    Asserts the written rows bit-identical between the fills and the guards intact; returns the garbage run's Guarded."""
    runs = [attn_launch(mode, with_tails(qkv, lens_of_tails, junk), out_rows, junk, **tables) for junk in (False, True)]
    for o in runs:
        assert o.guards_intact(), mode
    for b, (r0, n, _) in enumerate(spans):
        assert torch.equal(runs[0].bits[r0:r0 + n], runs[1].bits[r0:r0 + n]), (mode, b, "what nobody wrote changed a valid row")
    return runs[1]


def check_rows(mode, out, refs, spans, what):
    vals = attn_values(mode, out)
    worst = 0.0
    for b, (r0, n, _) in enumerate(spans):
        assert torch.isfinite(vals[r0:r0 + n]).all(), (mode, b)
        worst = max(worst, (vals[r0:r0 + n].double() - refs[b]).abs().max().item())
    print(f"[launch forms: attention {mode}] {what}: Linf vs float64 of the rounded operands {worst:.2e}")
    assert worst < AMODES[mode][3], (mode, what)


def untouched(out, written):
    """True where no span (first row, _, rows written) covers the row: those rows must still hold the sentinel."""
    keep = torch.ones(out.shape[0], dtype=torch.bool, device=DEV)
    for r0, _, n in written:
        keep[r0:r0 + n] = False
    return bool((out.bits[keep] == out.sent).all())


@pytest.mark.parametrize("B,H,N,lens", PACKED_SHAPES)
@pytest.mark.parametrize("mode", list(AMODES))
def test_attention_packed_rows_on_a_shared_length_table(mode, B, H, N, lens):
    """Bp = 2B batch rows, nlens = B (both CFG halves read lens[b % B]), kv_lens = q_lens = lens, packed output rows: the valid rows
    of every batch row match the row computed alone; nothing is written past min(N, span) of a row or past row_start[Bp]."""
    Bp = 2 * B
    qkv = attn_inputs(Bp, H, N, seed=N + H)
    rs = LO.row_start(lens)
    spans = [(rs[b], lens[b % B], min(N, rs[b + 1] - rs[b])) for b in range(Bp)]
    out = attn_case(mode, qkv, lens, rs[Bp] + EXTRA, spans, kv_lens=lens, q_lens=lens, row_start=rs)
    refs = LO.attention_alone(*LO.as_operands(mode, *qkv), lens, lens)
    check_rows(mode, out, refs, spans, f"packed B={B} H={H} N={N}")
    assert untouched(out, spans), (mode, "rows past a span or past row_start[Bp] were written")


@pytest.mark.parametrize("mode", list(AMODES))
def test_attention_padded_rows_with_q_lens(mode):
    """No row_start: rows below len match the reference; the 128-row query blocks wholly past len (len = 37: the block at row 128)
    exit before they load anything and leave the sentinel."""
    B, H, N, lens = PACKED_SHAPES[0]
    Bp = 2 * B
    qkv = attn_inputs(Bp, H, N, seed=5)
    spans = [(b * N, lens[b % B], min(N, (lens[b % B] + 127) // 128 * 128)) for b in range(Bp)]
    out = attn_case(mode, qkv, lens, Bp * N, spans, kv_lens=lens, q_lens=lens)
    refs = LO.attention_alone(*LO.as_operands(mode, *qkv), lens, lens)
    check_rows(mode, out, refs, spans, "padded with q_lens")
    assert untouched(out, spans), (mode, "a query block wholly past len was computed")


@pytest.mark.parametrize("mode", ["bf16", "f16", "attn16"])
def test_attention_tile_rotation_classes(mode):
    """attn2_fwd_kernel rotates three LDS stages; its remainder code has six (nfull % 3, edge tile or not) classes:
    kv_len 64, 128, 192 (nfull = 1, 2, 3, no edge tile) and 70, 130, 200 (the same with one), all in one launch, every query kept."""
    kv = [64, 128, 192, 70, 130, 200]
    Bp, H, N = 6, 2, 320
    qkv = attn_inputs(Bp, H, N, seed=7)
    spans = [(b * N, N, N) for b in range(Bp)]
    runs = [attn_launch(mode, [qkv[0]] + with_tails(qkv[1:], kv, junk), Bp * N, junk, kv_lens=kv) for junk in (False, True)]
    assert torch.equal(runs[0].bits, runs[1].bits), (mode, "keys past kv_len changed the output")
    assert runs[1].guards_intact()
    refs = LO.attention_alone(*LO.as_operands(mode, *qkv), kv, None)
    check_rows(mode, runs[1], refs, spans, "tile rotation")


@pytest.mark.parametrize("hi", [0, 3])
def test_split_kernel_planar_store_is_the_split_of_its_plain_store(hi):
    """o_planar = 1 (what the out-projection reads as a pre-split A operand; with qk_norm: hi_only = 3) holds exactly the hi / lo
    halves of the o_planar = 0 output, row for row."""
    B, H, N, lens = PACKED_SHAPES[0]
    mode = "f16x3/hi3" if hi else "f16x3"
    qkv = attn_inputs(2 * B, H, N, seed=11)
    rs = LO.row_start(lens)
    plain, planar = (attn_launch(mode, qkv, rs[-1] + EXTRA, True, o_planar=p, kv_lens=lens, q_lens=lens, row_start=rs) for p in (0, 1))
    assert planar.guards_intact()
    for b in range(2 * B):
        r0, n = rs[b], min(N, rs[b + 1] - rs[b])
        assert torch.equal(planar.bits[r0:r0 + n], split_planar64(plain.value[r0:r0 + n])), b
    assert (planar.bits[rs[-1]:] == planar.sent).all()


def test_attn16_planes_against_the_f16_kernel():
    """attn16 = the f16 v2 kernel storing through store4_planar.  split4_f16 (f5_common.h) takes hi = the f32 value converted to
    f16 by __builtin_convertvector (round to nearest even) -- the conversion store4(f16_t*) applies to the same value -- so the hi
    plane must hold the plain f16 mode's output bits, and hi + lo (22 bits of the f32 value) keeps the f16 kernel's bound."""
    B, H, N, lens = PACKED_SHAPES[0]
    qkv = attn_inputs(2 * B, H, N, seed=13)
    rs = LO.row_start(lens)
    spans = [(rs[b], lens[b % B], min(N, rs[b + 1] - rs[b])) for b in range(2 * B)]
    o16, opl = (attn_launch(m, qkv, rs[-1] + EXTRA, True, kv_lens=lens, q_lens=lens, row_start=rs) for m in ("f16", "attn16"))
    hi, lo = planar_planes(opl.bits)
    for r0, _, n in spans:
        assert torch.equal(hi[r0:r0 + n].view(torch.int16), o16.bits[r0:r0 + n])
        assert (lo[r0:r0 + n].float().abs() <= hi[r0:r0 + n].float().abs() * 2.0 ** -11 + 2.0 ** -25).all()   # half an f16 ulp of hi
    check_rows("attn16", opl, LO.attention_alone(*LO.as_operands("attn16", *qkv), lens, lens), spans, "Of planes")


@pytest.mark.parametrize("mode", list(AMODES))
def test_attention_launch_forms_are_deterministic(mode):
    """Race detector on the packed form (early-exit blocks next to running ones, the pair merge through the reused ring)."""
    B, H, N, lens = PACKED_SHAPES[0]
    qkv = with_tails(attn_inputs(2 * B, H, N, seed=17), lens, True)
    rs = LO.row_start(lens)
    first = attn_launch(mode, qkv, rs[-1] + EXTRA, True, kv_lens=lens, q_lens=lens, row_start=rs)
    for _ in range(2):
        again = attn_launch(mode, qkv, rs[-1] + EXTRA, True, kv_lens=lens, q_lens=lens, row_start=rs)
        assert torch.equal(again.raw, first.raw), mode


# ------------------------------------------------------------------------------------------------------- conv-pos
CONV_PRECS = ["f32", "f16x3", "bf16", "f16"]
CONV_DIMS = [256, 512, 768, 1024]


def conv_weights(D, seed):
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(D, D // 16, 31, generator=g) * (1.0 / (31 * D / 16) ** 0.5)).to(DEV)
    return w, torch.randn(D, generator=g).to(DEV)


def conv_case(prec, D, B, N, lens, packed, with_res, seed):
    """One conv-pos launch form, both fills of the x rows past each length; asserts everything the form promises."""
    Bp = 2 * B
    g = torch.Generator().manual_seed(seed)
    w, bias = conv_weights(D, seed)
    rs = LO.row_start(lens) if packed else [b * N for b in range(Bp + 1)]
    rows = rs[Bp] + (EXTRA if packed else 0)
    valid = torch.randn(rows, D, generator=g).to(DEV)
    res = torch.randn(rows, D, generator=g).to(DEV) if with_res else None
    dead = torch.ones(rows, dtype=torch.bool, device=DEV)      # x rows no utterance owns: pad rows of a span, rows past a length
    for b in range(Bp):
        dead[rs[b]:rs[b] + lens[b % B]] = False
    ys = []
    for junk in (False, True):
        x = valid.clone()
        x[dead] = garbage((rows, D), seed + 1)[dead] if junk else 0.0
        y = Guarded((rows, D), torch.float32)
        k_convpos_ex(prec, x, w, bias, res, y, Bp, N, lens=lens, row_start=rs if packed else None)
        assert y.guards_intact()
        ys.append(y)
    assert torch.equal(ys[0].bits, ys[1].bits), "x rows past a length changed the output"
    y = ys[1]
    worst, scale = 0.0, 1.0
    for b in range(Bp):
        r0, n, end = rs[b], lens[b % B], rs[b + 1]
        ref = LO.convpos_alone(prec, valid[r0:r0 + n], w, bias, None if res is None else res[r0:r0 + n])
        scale = max(scale, ref.abs().max().item())
        worst = max(worst, (y.value[r0:r0 + n].double() - ref).abs().max().item())
        if res is None:
            assert (y.bits[r0 + n:end] == 0).all(), (b, "rows [len, span) without res must be +0")
        else:
            assert torch.equal(y.value[r0 + n:end], res[r0 + n:end]), (b, "rows [len, span) must equal res")
    assert (y.bits[rs[Bp]:] == y.sent).all(), "rows past row_start[Bp] were written"
    print(f"[launch forms: convpos {prec}] D={D} B={B} N={N} packed={packed} res={with_res}: Linf {worst:.2e} (|ref|max {scale:.2f})")
    assert worst < 5e-5 * scale


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("prec", CONV_PRECS)
@pytest.mark.parametrize("D", CONV_DIMS)
def test_convpos_packed_masked_on_a_shared_length_table(D, prec, with_res):
    """Packed rows: the neighbours of an utterance's rows are another utterance's REAL rows, so a halo that leaks past the item's
    own ends fails the comparison with the item convolved alone (len = 5 is shorter than the 15-row halo on both sides)."""
    conv_case(prec, D, 3, 150, [150, 97, 5], True, with_res, seed=D + 1)


@pytest.mark.parametrize("lens", [[150, 97, 5], [128, 129, 1]])
@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("prec", CONV_PRECS)
@pytest.mark.parametrize("D", CONV_DIMS)
def test_convpos_padded_masked(D, prec, with_res, lens):
    """Padded rows: rows at or past len equal res (or 0); lens 128 / 129 end on and one past the 128-token tile."""
    conv_case(prec, D, 3, 150, lens, False, with_res, seed=D + 2)


RING_LENS = [130, 128, 1, 64, 129, 100, 17, 130, 127, 5, 96, 33, 2]


@pytest.mark.parametrize("prec,D,packed", [("f32", 256, False), ("bf16", 256, False), ("f16", 256, False), ("f16", 256, True),
                                           ("f16x3", 1024, False)])
def test_convpos_four_stage_weight_ring(prec, D, packed):
    """2 tiles x 16 groups x 26 batch rows = 832 blocks > 384: launch_convpos_cpg picks the 4-stage ring (NS = 4), which no
    smaller batch reaches; D = 1024 under f16x3 is the split kernel's."""
    conv_case(prec, D, 13, 130, RING_LENS, packed, True, seed=D + 3)
