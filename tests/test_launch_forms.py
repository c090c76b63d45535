"""CPU: the references of tests/test_launch_forms_gpu.py (launch_oracle: every batch row computed alone) against the masked
whole-batch formulations the older kernel tests use, in float64 -- so that the GPU tests compare the kernels with the operation
itself and not with a second mistake."""
import torch
import torch.nn.functional as F

import launch_oracle as LO


def test_attention_alone_equals_masked_sdpa_of_the_padded_batch():
    g = torch.Generator().manual_seed(1)
    B, H, N = 3, 2, 70
    lens = [70, 37, 1]
    q, k, v = (torch.randn(2 * B, H, N, 64, generator=g, dtype=torch.float64) for _ in range(3))
    for t in (q, k, v):                       # what lies past a row's length must not matter to either side
        for b in range(2 * B):
            t[b, :, lens[b % B]:] = 1e3
    keep = torch.arange(N)[None, :] < torch.tensor(lens * 2)[:, None]                     # [Bp, N]: the CFG halves share the table
    ref = F.scaled_dot_product_attention(q, k, v, attn_mask=keep[:, None, None, :])        # [Bp, H, N, 64], scale 64^-0.5
    ref = ref.transpose(1, 2).reshape(2 * B, N, H * 64)
    alone = LO.attention_alone(q, k, v, lens, lens)
    for b in range(2 * B):
        n = lens[b % B]
        assert alone[b].shape == (n, H * 64)
        assert (alone[b] - ref[b, :n]).abs().max() < 1e-12
    # keys masked, every query kept (the tile rotation case)
    full = LO.attention_alone(q, k, v, lens, None)
    for b in range(2 * B):
        assert full[b].shape == (N, H * 64) and (full[b] - ref[b]).abs().max() < 1e-12


def test_attention_operand_rounding_per_mode():
    g = torch.Generator().manual_seed(2)
    q, k, v = (torch.randn(1, 1, 8, 64, generator=g) for _ in range(3))
    for mode in ("f32", "f16x3"):
        assert all(a is b for a, b in zip(LO.as_operands(mode, q, k, v), (q, k, v)))
    qs = 0.125 * LO.L2E
    for mode, dt in (("bf16", torch.bfloat16), ("f16", torch.float16), ("attn16", torch.float16)):
        qr, kr, vr = LO.as_operands(mode, q, k, v)
        assert torch.equal((qr * qs).to(dt), (q * qs).to(dt)) and torch.equal(kr, k.to(dt).float()) and torch.equal(vr, v.to(dt).float())
    q1, k1, v1 = LO.as_operands("f16x3/hi1", q, k, v)
    q2, k2, v2 = LO.as_operands("f16x3/hi2", q, k, v)
    q3, k3, v3 = LO.as_operands("f16x3/hi3", q, k, v)
    assert torch.equal(q1 * 0.125, (q * 0.125).half().float()) and torch.equal(k1, k.half().float()) and v1 is v
    assert q2 is q and k2 is k and torch.equal(v2, v.half().float())
    assert torch.equal(q3, q1) and torch.equal(k3, k1) and torch.equal(v3, v2)


def test_convpos_alone_equals_the_masked_conv1d_formulation():
    g = torch.Generator().manual_seed(3)
    B, N, D = 3, 60, 256
    lens = [60, 37, 5]                        # 5 < the 15-row halo
    x = torch.randn(B, N, D, generator=g, dtype=torch.float64)
    w = torch.randn(D, 16, 31, generator=g, dtype=torch.float64) * 0.05
    bias = torch.randn(D, generator=g, dtype=torch.float64)
    res = torch.randn(B, N, D, generator=g, dtype=torch.float64)
    m = (torch.arange(N)[None] < torch.tensor(lens)[:, None])[:, None]                     # [B, 1, N], as test_convpos_masked_rows
    h = x.permute(0, 2, 1).masked_fill(~m, 0.0)
    h = F.conv1d(h, w, bias, padding=15, groups=16).masked_fill(~m, 0.0)
    ref = F.mish(h).permute(0, 2, 1)
    for b in range(B):
        n = lens[b]
        assert (LO.convpos_alone("f32", x[b, :n], w, bias) - ref[b, :n]).abs().max() < 1e-12
        assert (LO.convpos_alone("f32", x[b, :n], w, bias, res[b, :n]) - (ref[b, :n] + res[b, :n])).abs().max() < 1e-12
        assert (ref[b, n:] == 0).all()         # what the kernel must write for rows [len, span): mish(0) = 0 (+ res)


def test_row_start_follows_the_engine_rule():
    """engine_impl.h: t[q + 1] = t[q] + round_up(lens[q % B], 4) over halves * B batch rows; row_start[Bp] is the row count."""
    assert LO.row_start([200, 37, 129]) == [0, 200, 240, 372, 572, 612, 744]
    assert LO.row_start([150, 97, 5]) == [0, 152, 252, 260, 412, 512, 520]
    assert LO.row_start([256, 70], halves=1) == [0, 256, 328]
    for lens in ([1], [3, 4, 5], [130, 128, 1, 64, 129]):
        rs = LO.row_start(lens)
        assert len(rs) == 2 * len(lens) + 1 and rs[0] == 0
        for b in range(2 * len(lens)):
            span = rs[b + 1] - rs[b]
            assert rs[b] % 4 == 0 and span % 4 == 0 and 0 <= span - lens[b % len(lens)] < 4
        assert rs[-1] == 2 * sum((n + 3) // 4 * 4 for n in lens)


def test_planar_planes_reads_back_what_split_planar64_writes():
    from gpu_util import planar_planes, split_planar64
    g = torch.Generator().manual_seed(4)
    x = torch.randn(5, 128, generator=g)
    hi, lo = planar_planes(split_planar64(x))
    assert torch.equal(hi, x.half()) and torch.equal(lo, (x - x.half().float()).half())
    assert (hi.float() + lo.float() - x).abs().max() < 2.0 ** -21 * x.abs().max()


def test_entry_points_refuse_forms_that_do_not_exist():
    """Argument validation comes before the first HIP call, so it runs without a GPU (the data pointers are never read)."""
    import ctypes as C

    from f5_tts_amd import _lib
    lib = _lib.load()
    fake = C.c_void_p(64)
    Bp, H, N = 4, 2, 100

    def attn(prec, **kw):
        p = _lib.f5k_attn()
        p.out, p.n_out = 64, Bp * N * H * 64
        keep = []
        for name, val in kw.items():
            if name.endswith("_host"):
                val = _lib.int_array(val)
                keep.append(val)
            setattr(p, name, val)
        rc = lib.f5k_attention_ex(_lib.PRECISIONS[prec], fake, fake, fake, Bp, H, N, C.byref(p), None)
        return rc, lib.f5_last_error().decode()

    for prec, kw, word in [("bf16", dict(mode=1), "mode 1"), ("f16x3", dict(mode=2), "mode"), ("f16", dict(hi_only=1), "hi_only"),
                           ("f32", dict(o_planar=1), "o_planar"), ("f16x3", dict(mode=1, hi_only=3), "hi_only"),
                           ("f16x3", dict(hi_only=4), "hi_only"), ("f16p", dict(), "precision"),
                           ("f32", dict(vt_pad_fill=float("nan")), "finite"), ("f32", dict(vt_pad_fill=float("inf")), "finite"),
                           ("f32", dict(kv_lens_host=[100, 50], nlens=0), "nlens"), ("f32", dict(q_lens_host=[1] * 5, nlens=5), "nlens"),
                           ("f32", dict(row_start_host=[0, 100, 202, 300, 400]), "row_start"),
                           ("f32", dict(row_start_host=[4, 104, 204, 304, 404]), "row_start"),
                           ("f32", dict(row_start_host=[0, 104, 208, 312, 416]), "row_start"),
                           ("f32", dict(n_out=Bp * N * H * 64 - 1), "smaller")]:
        rc, msg = attn(prec, **kw)
        assert rc == -1 and word in msg and msg.startswith("f5k_attention_ex"), (prec, kw, msg)

    def conv(D, lens, rs, rows):
        p = _lib.f5k_conv()
        la, ra = _lib.int_array(lens), _lib.int_array(rs)
        if la is not None:
            p.lens_host, p.nlens = la, len(lens)
        if ra is not None:
            p.row_start_host = ra
        p.rows = rows
        rc = lib.f5k_convpos_ex(0, fake, fake, fake, None, fake, Bp, N, D, C.byref(p), None)
        return rc, lib.f5_last_error().decode()

    for D, lens, rs, rows, word in [(300, None, None, 400, "D must"), (256, [50] * 5, None, 400, "nlens"), (256, [-1, 5], None, 400, "negative"),
                                    (256, [50, 9], [0, 52, 60, 112, 120], 120, "row_start"),     # 9 rows do not fit a span of 8
                                    (256, [50, 9], [0, 52, 64, 116, 128], 127, "fewer rows"), (256, None, None, 399, "fewer rows")]:
        rc, msg = conv(D, lens, rs, rows)
        assert rc == -1 and word in msg and msg.startswith("f5k_convpos_ex"), (D, lens, rs, msg)
