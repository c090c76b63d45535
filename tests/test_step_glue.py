"""CPU: the restatements of tests/glue_oracle.py against independent formulations, and the conditions the cases of
tests/test_step_glue_gpu.py rely on (they reach the loop's second pass, alignment rows, frames past a length, idle lanes)."""
import torch
import torch.nn.functional as F

import glue_oracle as G
import ode_oracle
from oracle import f5_oracle as O


def test_xrmsnorm_oracle_is_normalize_times_sqrt_d_times_g():
    g0 = torch.Generator().manual_seed(0)
    for D in G.XRMS_DIMS:
        x = torch.randn(G.XRMS_ROWS, D, generator=g0, dtype=torch.float64)
        g = torch.randn(D, generator=g0, dtype=torch.float64)
        x[3] = 0
        ref = F.normalize(x, dim=-1) * D ** 0.5 * g
        got = G.xrmsnorm(x, g)
        assert torch.allclose(got, ref, rtol=1e-14, atol=0) and not got[3].any()
        assert torch.allclose(got, O.x_rmsnorm(x, g), rtol=1e-14, atol=0)


def test_ode_oracles_step_a_linear_field_like_the_fixed_grid_solvers():
    """dy/dt = a y + c t through the step oracles equals ode_oracle.fixed_grid_odeint on the f32 grid (state in float64, dt the f32
    difference in both; the same operations up to the association of the half step, hence the 1e-15 tolerance)."""
    tg = G.sway_grid(8)
    assert (tg[1:] - tg[:-1]).unique().numel() > 4, "the grid must not be uniform"
    g0 = torch.Generator().manual_seed(1)
    y0 = torch.randn(2, 5, 8, generator=g0, dtype=torch.float64)
    a, c = -0.7, 0.3
    fn = lambda tt, y: a * y + c * tt   # noqa: E731
    for method in ode_oracle.METHODS:
        ref = ode_oracle.fixed_grid_odeint(fn, y0, tg, method)
        assert ref.dtype == torch.float64
        y = y0
        for i in range(8):
            if method == "euler":
                y = G.euler_step(y, fn(tg[i], y), None, tg, i, 0.0)
            else:
                y_mid = G.midpoint_half_step(y, fn(tg[i], y), None, tg, i, 0.0)
                y = G.euler_step(y, fn(tg[i] + 0.5 * (tg[i + 1] - tg[i]), y_mid), None, tg, i, 0.0)
            assert torch.allclose(y, ref[i + 1], rtol=1e-15, atol=1e-15), (method, i)


def test_velocity_is_the_cfg_mix_and_keep_freezes_frames():
    g0 = torch.Generator().manual_seed(2)
    p, u, y = (torch.randn(3, 12, 8, generator=g0) for _ in range(3))
    assert torch.equal(G.velocity(p, u, 2.0), p.double() + (p.double() - u.double()) * 2.0)
    assert torch.equal(G.velocity(p, None, 2.0), p.double())
    tg = G.sway_grid(8)
    keep = G.frame_mask(G.PACKED["lens"], G.PACKED["N"])
    out = G.euler_step(y, p, u, tg, 3, 2.0, keep)
    full = G.euler_step(y, p, u, tg, 3, 2.0)
    for b, n in enumerate(G.PACKED["lens"]):
        assert torch.equal(out[b, :n], full[b, :n]) and torch.equal(out[b, n:], y[b, n:].double())


def test_pack_oracle_is_cat_plus_the_cfg_packing_of_the_model_oracle(monkeypatch):
    """oracle.f5_oracle.input_embed with an identity projection and no position embedding IS its torch.cat; dit_forward packs the CFG batch
    as cat((embed(cond, text), embed(no cond, dropped text)), dim=0) (f5_oracle.py dit_forward)."""
    g0 = torch.Generator().manual_seed(3)
    B, N, mel, Dt = 2, 5, 8, 4
    x, cond = (torch.randn(B, N, mel, generator=g0, dtype=torch.float64) for _ in range(2))
    tc, tu = (torch.randn(B, N, Dt, generator=g0, dtype=torch.float64) for _ in range(2))
    W = {"input_embed.proj.weight": torch.eye(2 * mel + Dt, dtype=torch.float64)}
    monkeypatch.setattr(O, "conv_pos_embed", lambda W, pfx, h, mask=None: torch.zeros_like(h))
    embed = lambda drop, text: O.input_embed(W, x, cond, text, drop_audio_cond=drop)   # noqa: E731
    assert torch.equal(G.pack_input(x, cond, tc, tu, 2 * B), torch.cat((embed(False, tc), embed(True, tu)), dim=0))
    assert torch.equal(G.pack_input(x, cond, tc, tu, B), torch.cat((x, cond, tc), dim=-1))
    assert torch.equal(G.pack_input(x, cond, tu, tu, B, True), embed(True, tu))


def test_row_tables_and_packing_round_trip():
    lens, N = [5, 1, 8], 8
    rs = G.row_start_table(lens, 2)
    assert rs == [0, 8, 12, 20, 28, 32, 40]
    rm = G.rowmap_table(rs)
    assert rm.shape == (40, 2) and rm[8].tolist() == [1, 0] and rm[39].tolist() == [5, 7] and rm[27].tolist() == [3, 7]
    padded = torch.arange(6 * N * 3, dtype=torch.float32).reshape(6, N, 3) + 1
    rows = G.pack_rows(padded, rs, lens)
    for r, (bp, n) in enumerate(rm.tolist()):
        want = padded[bp, n] if n < lens[bp % 3] else torch.zeros(3)
        assert torch.equal(rows[r], want)
    for half in range(2):
        back = G.unpack_rows(rows, rs, lens, half, 3, N)
        for b in range(3):
            assert torch.equal(back[b, :lens[b]], padded[half * 3 + b, :lens[b]]) and not back[b, lens[b]:].any()


def test_small_oracles():
    g0 = torch.Generator().manual_seed(4)
    a, b = torch.randn(6, 8, generator=g0), torch.randn(6, 8, generator=g0)
    m = torch.tensor([1, 0, 0, 1, 1, 0], dtype=torch.uint8)
    assert torch.equal(G.select_rows(a, b, m)[m.bool()], a[m.bool()]) and torch.equal(G.select_rows(a, None, m)[~m.bool()], torch.zeros(3, 8))
    t = torch.tensor([0.0, 1.0, 0.37], dtype=torch.float32)
    assert torch.allclose(G.time_sinus(t, G.time_freqs()).float(), O.sinus_features(t), atol=1e-6)
    h, temb = torch.randn(3, 5, 64, generator=g0), torch.randn(3, 64, generator=g0)
    x = G.unett_assemble(h, temb, 64)
    assert torch.equal(x[:, 0], temb) and torch.equal(x[:, 1:], h) and torch.equal(G.strip_first_token(x), h)
    assert torch.equal(G.unett_assemble(h, temb, 0)[:, 0], temb[:1].expand(3, 64))


def test_the_gpu_cases_reach_what_they_are_there_for():
    for name in G.STRIDED:
        assert G.strided_items(name) > G.EW_CAP_ITEMS, f"{name}: the loop's second pass is not reached"
        assert G.strided_items(name) < 2 * G.EW_CAP_ITEMS, f"{name}: larger than the second pass needs"
    for lens in (G.PACKED["lens"], G.STRIDED["euler_packed"]["lens"], G.STRIDED["midpoint_packed"]["lens"]):
        assert any(n % 4 for n in lens), "no alignment row"
    assert any(n < G.PACKED["N"] for n in G.PACKED["lens"]) and any(n < 14000 for n in G.STRIDED["euler_packed"]["lens"]), "no frame past a length"
    assert 68 in G.XRMS_DIMS and 68 // 4 < 64, "D = 68 must leave lanes of the wave without data"
    assert G.XRMS_ROWS % 4, "the last block of four rows must be partial"
    p = G.pattern((2, 1024), 1)
    assert p.abs().max() <= 64 and torch.equal(p * 8, (p * 8).round()) and (p[:, 1:] != p[:, :-1]).all()
