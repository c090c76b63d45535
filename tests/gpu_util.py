"""Helpers for the -m gpu tests: call the kernel-level C entry points on torch device tensors."""
import ctypes as C

import torch

from f5_tts_amd import _lib

DEV = "cuda:0"


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def prec_id(name):
    return _lib.PRECISIONS[name]


def k_gemm(prec, A, W, bias=None, act=0, tile=(0, 0)):
    lib = _lib.load()
    M, K = A.shape
    N = W.shape[0]
    out = torch.empty(M, N, device=A.device, dtype=torch.float32)
    _lib.check(lib.f5k_gemm(prec_id(prec), _p(A), _p(W), _p(bias), act, _p(out), M, N, K, tile[0], tile[1], _s()), "f5k_gemm")
    return out


def k_gemm_plan(elem_size, M, N, K, has_m_limit=0, m_hint=0, form=0, conv=0, pp_epi=1, force_cfg=-1, env_cfg=-1, env_n=0):
    """launch_gemm's decision (f5k_gemm_plan, no GPU needed): [] nothing to do, None refused, else a list of
    (family, tile, first row, rows)."""
    plan = (C.c_int32 * 9)()
    _lib.check(_lib.load().f5k_gemm_plan(elem_size, M, N, K, has_m_limit, m_hint, form, conv, pp_epi, force_cfg, env_cfg, env_n, plan),
               "f5k_gemm_plan")
    return None if plan[0] < 0 else [tuple(plan[1 + 4 * i:5 + 4 * i]) for i in range(plan[0])]


def k_attention(prec, q, k, v, lens=None):
    lib = _lib.load()
    Bp, H, N, _ = q.shape
    out = torch.empty(Bp, N, H * 64, device=q.device, dtype=torch.float32)
    _lib.check(lib.f5k_attention(prec_id(prec), _p(q), _p(k), _p(v), _lib.int_array(lens), _p(out), Bp, H, N, _s()),
               "f5k_attention")
    return out


def k_convpos(prec, x, w, bias, res=None, lens=None):
    lib = _lib.load()
    Bp, N, D = x.shape
    y = torch.empty_like(x)
    _lib.check(lib.f5k_convpos(prec_id(prec), _p(x), _p(w), _p(bias), _p(res), _lib.int_array(lens), _p(y), Bp, N, D, _s()),
               "f5k_convpos")
    return y


def k_layernorm_mod(x, scale, shift, rows_per_batch, eps=1e-6):
    lib = _lib.load()
    R, D = x.shape
    out = torch.empty_like(x)
    _lib.check(lib.f5k_layernorm_mod(_p(x), _p(scale), _p(shift), _p(out), R, D, rows_per_batch, eps, _s()), "f5k_layernorm_mod")
    return out


# ---- guarded output buffers and the production-epilogue entry points (tests/test_epilogues_gpu.py)
SENT32 = 0x7FA5A5A5   # a NaN in f32
SENT16 = 0x7FA5       # a NaN in both f16 and bf16
GUARD = 64            # elements of sentinel before and after every buffer (keeps 128-byte alignment)


class Guarded:
    """A device buffer of `shape` x `dtype` between two guard bands, all filled with a NaN sentinel before the launch."""

    def __init__(self, shape, dtype):
        self.shape, self.dtype = tuple(shape), dtype
        self.n = 1
        for s in self.shape:
            self.n *= s
        wide = dtype == torch.float32
        self.sent = SENT32 if wide else SENT16
        self.raw = torch.full((2 * GUARD + self.n,), self.sent, dtype=torch.int32 if wide else torch.int16, device=DEV)

    @classmethod
    def like(cls, t):
        """A guarded copy of f32 tensor t (e.g. a residual that the epilogue updates in place)."""
        g = cls(t.shape, torch.float32)
        g.value.copy_(t)
        return g

    @property
    def bits(self):
        return self.raw[GUARD:GUARD + self.n].view(self.shape)

    @property
    def value(self):
        return self.raw[GUARD:GUARD + self.n].view(self.dtype).view(self.shape)

    def ptr(self):
        return self.raw.data_ptr() + GUARD * self.raw.element_size()

    def guards_intact(self):
        return bool((self.raw[:GUARD] == self.sent).all() and (self.raw[GUARD + self.n:] == self.sent).all())


def k_layernorm_mod_ex(prec, x, scale, shift, out, rows_per_batch, m_limit=-1, planar=0, eps=1e-6):
    """out: a Guarded of [R, D] (f32 for f32 / f16x3, else the 16-bit type); returns its values as f32."""
    lib = _lib.load()
    R, D = x.shape
    cpy = None if out.dtype == torch.float32 else torch.empty(R, D, device=DEV)
    _lib.check(lib.f5k_layernorm_mod_ex(prec_id(prec), _p(x), _p(scale), _p(shift), C.c_void_p(out.ptr()), _p(cpy), R, D,
                                        rows_per_batch, eps, m_limit, planar, _s()), "f5k_layernorm_mod_ex")
    return out.value if cpy is None else cpy


def k_gemm_epi(prec, A, W, bias, kind, outs, *, cfg=-1, a_presplit=False, m_limit=-1, out16=False, act=0, planar=0, res=None,
               gate=None, gate_stride=0, rows_per_batch=1, lens=None, H=0, Nseq=0, Npad=0, pe_heads=0, q_scale=1.0, rope_cos=None,
               rope_sin=None, row_start=None, Bp=0, gq=None, gk=None):
    """One GEMM through a production epilogue (f5k_gemm_epi).  outs: Guarded buffers (STORE / GATE_RES: [out]; QKV: [q, k, vt]).
    Returns their values as f32 (16-bit outputs through the library's to_f32_kernel)."""
    lib = _lib.load()
    M, K = A.shape
    N = W.shape[0]
    p = _lib.f5k_epi()
    p.kind, p.cfg, p.a_presplit, p.m_limit, p.out16, p.act, p.planar = kind, cfg, int(a_presplit), m_limit, int(out16), act, planar
    p.gate_stride, p.rows_per_batch = gate_stride, rows_per_batch
    p.res = 0 if res is None else (res.ptr() if isinstance(res, Guarded) else res.data_ptr())
    p.gate = 0 if gate is None else gate.data_ptr()
    la = _lib.int_array(lens)
    if la is not None:
        p.lens_host, p.nlens = la, len(lens)
    p.H, p.Nseq, p.Npad, p.pe_heads, p.q_scale = H, Nseq, Npad, pe_heads, q_scale
    if rope_cos is not None:
        p.rope_cos, p.rope_sin, p.maxpos = rope_cos.data_ptr(), rope_sin.data_ptr(), rope_cos.shape[0]
    rs = _lib.int_array(row_start)
    if rs is not None:
        p.row_start_host = rs
    p.Bp = Bp
    p.gq = 0 if gq is None else gq.data_ptr()
    p.gk = 0 if gk is None else gk.data_ptr()
    cps = [None if o.dtype == torch.float32 else torch.empty(o.shape, device=DEV) for o in outs]
    for i, o in enumerate(outs):
        setattr(p, f"out{i}", o.ptr())
        if cps[i] is not None:
            setattr(p, f"out{i}_f32", cps[i].data_ptr())
            setattr(p, f"n{i}", o.n)
    _lib.check(lib.f5k_gemm_epi(prec_id(prec), _p(A), _p(W), _p(bias), M, N, K, C.byref(p), _s()), "f5k_gemm_epi")
    return [o.value if c is None else c for o, c in zip(outs, cps)]


# ---- the pre-split ("planar") f32 row layout of F5_PREC_F16X3, restated once for every test that reads it
def _planar_order(device):
    return torch.tensor([4 * g + s if s < 4 else 16 + 4 * g + s - 4 for g in range(4) for s in range(8)], device=device)


def split_planar64(x):
    """The layout split_planar_kernel writes, restated (per 32 floats: chunk g = f16 hi of k = 4g..4g+3, 16+4g..16+4g+3, chunk
    4 + g = the f16 lo of the same k) -- used to cross-check the library's own split of a plain store."""
    v = x.reshape(-1, 32)
    v = v[:, _planar_order(x.device)]
    hi = v.half()
    lo = (v - hi.float()).half()
    return torch.cat((hi, lo), dim=1).contiguous().view(torch.int32).view(x.shape)


def planar_planes(bits):
    """The inverse reading: int32 bits of pre-split rows -> (hi, lo) f16 tensors of the same shape in natural element order."""
    h = bits.contiguous().view(torch.int16).view(torch.float16).reshape(-1, 64)
    inv = torch.argsort(_planar_order(bits.device))
    return h[:, :32][:, inv].reshape(bits.shape), h[:, 32:][:, inv].reshape(bits.shape)


# ---- attention and conv-pos in the forms the engine launches them (tests/test_launch_forms_gpu.py)
def k_attention_ex(prec, q, k, v, out, *, kv_lens=None, q_lens=None, row_start=None, mode=0, hi_only=0, o_planar=0, vt_pad_fill=0.0):
    """f5k_attention_ex into the Guarded `out` ([rows, H * 64] of the mode's output type).  kv_lens / q_lens share one length."""
    lib = _lib.load()
    Bp, H, N, _ = q.shape
    p = _lib.f5k_attn()
    kl, ql, rs = _lib.int_array(kv_lens), _lib.int_array(q_lens), _lib.int_array(row_start)
    if kl is not None:
        p.kv_lens_host, p.nlens = kl, len(kv_lens)
    if ql is not None:
        p.q_lens_host, p.nlens = ql, len(q_lens)
    if rs is not None:
        p.row_start_host = rs
    p.mode, p.hi_only, p.o_planar, p.vt_pad_fill = mode, hi_only, o_planar, vt_pad_fill
    p.out, p.n_out = out.ptr(), out.n
    _lib.check(lib.f5k_attention_ex(prec_id(prec), _p(q), _p(k), _p(v), Bp, H, N, C.byref(p), _s()), "f5k_attention_ex")
    return out


def k_convpos_ex(prec, x, w, bias, res, y, Bp, N, *, lens=None, row_start=None):
    """f5k_convpos_ex: x / res f32 tensors and y a Guarded, all [rows, D] (rows = row_start[Bp] or more, or Bp * N)."""
    lib = _lib.load()
    rows, D = y.shape
    assert x.shape == (rows, D) and (res is None or res.shape == (rows, D))
    p = _lib.f5k_conv()
    la, rs = _lib.int_array(lens), _lib.int_array(row_start)
    if la is not None:
        p.lens_host, p.nlens = la, len(lens)
    if rs is not None:
        p.row_start_host = rs
    p.rows = rows
    _lib.check(lib.f5k_convpos_ex(prec_id(prec), _p(x), _p(w), _p(bias), _p(res), C.c_void_p(y.ptr()), Bp, N, D, C.byref(p), _s()),
               "f5k_convpos_ex")
    return y


# ---- the step glue of sample() (tests/test_step_glue_gpu.py): device tensors in, Guarded buffers out, nothing staged by the library
ELEM_DTYPE = {"f32": torch.float32, "f16x3": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def _a(t):
    """Device address of a tensor, a Guarded or None."""
    return C.c_void_p(0 if t is None else t.ptr() if isinstance(t, Guarded) else t.data_ptr())


def _f32(*ts):
    for t in ts:
        assert t is None or isinstance(t, Guarded) or (t.dtype == torch.float32 and t.is_contiguous() and t.is_cuda)


def k_fill_rowmap(row_start, rowmap, Bp):
    """row_start: device int32 [Bp + 1]; rowmap: a Guarded f32-sized [rows, 2] whose .bits are the (b', n) pairs."""
    assert row_start.dtype == torch.int32 and row_start.numel() == Bp + 1 and rowmap.shape[0] >= int(row_start[Bp])
    _lib.check(_lib.load().f5k_fill_rowmap(_a(row_start), _a(rowmap), Bp, _s()), "f5k_fill_rowmap")
    return rowmap


def k_pack_input(prec, x, cond, text_c, text_u, out, Bp, drop_cond_first=0, rowmap=None, row_limit=None, lens=None):
    """out: a Guarded [rows, ldo] of the precision's element type.  RowPack form: rowmap (Guarded or int32 tensor [rows, 2]),
    row_limit (device int32 [1]) and lens (device int32 [B])."""
    B, N, mel = x.shape
    Dt = text_c.shape[-1]
    _f32(x, cond, text_c, text_u)
    assert cond.shape == x.shape and text_c.shape == text_u.shape == (B, N, Dt) and out.dtype == ELEM_DTYPE[prec]
    rows, ldo = out.shape
    if rowmap is None:
        assert rows >= Bp * N
    else:
        lim = int(row_limit.item())
        assert row_limit.dtype == lens.dtype == torch.int32 and lens.numel() == B and lim <= min(rows, rowmap.shape[0], Bp * N)
    _lib.check(_lib.load().f5k_pack_input(prec_id(prec), _p(x), _p(cond), _p(text_c), _p(text_u), _a(out), ldo, B, Bp, N, mel, Dt,
                                          int(drop_cond_first), _a(rowmap), _a(row_limit), _a(lens), _s()), "f5k_pack_input")
    return out


def _ode_args(y, pred, row_start, lens, tgrid, step, use_cfg):
    B, N, mel = y.shape
    halves = 2 if use_cfg else 1
    _f32(pred, tgrid)
    assert 0 <= step < tgrid.numel() - 1
    if row_start is None:
        assert pred.numel() >= halves * B * N * mel
    else:
        assert row_start.dtype == lens.dtype == torch.int32 and row_start.numel() == halves * B + 1 and lens.numel() == B
        assert pred.shape[-1] == mel and pred.shape[0] >= int(row_start[-1])
    return B, N, mel


def k_euler_cfg(y, pred, tgrid, step, cfg, use_cfg, traj_slot=None, row_start=None, lens=None):
    """y: a Guarded [B, N, mel] updated in place; traj_slot: a Guarded of the same shape or None."""
    B, N, mel = _ode_args(y, pred, row_start, lens, tgrid, step, use_cfg)
    assert traj_slot is None or traj_slot.shape == y.shape
    _lib.check(_lib.load().f5k_euler_cfg(_a(y), _p(pred), B, N, mel, _a(row_start), _a(lens), _p(tgrid), step, float(cfg), int(use_cfg),
                                         _a(traj_slot), _s()), "f5k_euler_cfg")
    return y


def k_midpoint_half_cfg(y, pred, tgrid, step, cfg, use_cfg, y_mid, row_start=None, lens=None):
    """y: f32 tensor [B, N, mel]; y_mid: a Guarded of the same shape."""
    _f32(y)
    B, N, mel = _ode_args(y, pred, row_start, lens, tgrid, step, use_cfg)
    assert y_mid.shape == y.shape
    _lib.check(_lib.load().f5k_midpoint_half_cfg(_p(y), _p(pred), B, N, mel, _a(row_start), _a(lens), _p(tgrid), step, float(cfg),
                                                 int(use_cfg), _a(y_mid), _s()), "f5k_midpoint_half_cfg")
    return y_mid


def k_select_rows(a, b, rowmask, out):
    """out (a Guarded [rows, C]) = rowmask ? a : b; b None (zeros), a tensor, or `out` itself (the in-place use)."""
    rows, Cc = out.shape
    _f32(a, b)
    assert a.shape == (rows, Cc) and rowmask.dtype == torch.uint8 and rowmask.numel() == rows and (b is None or b.shape == (rows, Cc))
    _lib.check(_lib.load().f5k_select_rows(_p(a), _a(b), _p(rowmask), _a(out), rows, Cc, _s()), "f5k_select_rows")
    return out


def k_time_sinus(t, freq, feat):
    _f32(t, freq)
    S = t.numel()
    assert freq.numel() == 128 and feat.shape == (S, 256)
    _lib.check(_lib.load().f5k_time_sinus(_p(t), _p(freq), _a(feat), S, _s()), "f5k_time_sinus")
    return feat


def k_xrmsnorm(prec, x, g, out, planar=0):
    R, D = x.shape
    _f32(x, g)
    assert g.numel() == D and out.shape == (R, D) and out.dtype == ELEM_DTYPE[prec]
    _lib.check(_lib.load().f5k_xrmsnorm(prec_id(prec), _p(x), _a(out), R, D, _p(g), planar, _s()), "f5k_xrmsnorm")
    return out


def k_unett_assemble(h, temb, temb_stride, x):
    Bp, N, D = h.shape
    _f32(h, temb)
    assert x.shape == (Bp, N + 1, D) and temb.numel() >= (Bp - 1) * temb_stride + D
    _lib.check(_lib.load().f5k_unett_assemble(_p(h), _p(temb), temb_stride, _a(x), Bp, N, D, _s()), "f5k_unett_assemble")
    return x


def k_cat2(prec, x, skip, out, planar=0):
    rows, D = x.shape
    _f32(x, skip)
    assert skip.shape == x.shape and out.shape == (rows, 2 * D) and out.dtype == ELEM_DTYPE[prec]
    _lib.check(_lib.load().f5k_cat2(prec_id(prec), _p(x), _p(skip), _a(out), rows, D, planar, _s()), "f5k_cat2")
    return out


def k_strip_first_token(inp, out):
    Bp, N1, Cc = inp.shape
    _f32(inp)
    assert out.shape == (Bp, N1 - 1, Cc)
    _lib.check(_lib.load().f5k_strip_first_token(_p(inp), _a(out), Bp, N1 - 1, Cc, _s()), "f5k_strip_first_token")
    return out


def k_work_plan(cfg, B, N, S, call_B, call_N):
    """f5k_work_plan (no GPU needed): (total bytes, {name: byte offset or None}, the same for the split-CFG side chain)."""
    n = len(_lib.F5K_WORK_NAMES)
    total, main, side = C.c_int64(), (C.c_int64 * n)(), (C.c_int64 * n)()
    _lib.check(_lib.load().f5k_work_plan(C.byref(cfg), B, N, S, call_B, call_N, C.byref(total), main, side), "f5k_work_plan")
    as_dict = lambda a: {k: (None if v < 0 else v) for k, v in zip(_lib.F5K_WORK_NAMES, a)}   # noqa: E731
    return total.value, as_dict(main), as_dict(side)
