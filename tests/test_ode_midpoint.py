"""CPU: the midpoint ODE solver of CFM.sample (odeint_kwargs=dict(method="midpoint")).

The public surface accepts it, the test-side solver (tests/ode_oracle.py) is pinned on closed-form ODEs and on the
oracle's own Euler, and the reference-generated fixtures (tools/make_golden_ode.py) are checked to be reproducible and
able to tell the midpoint rule from the two ways it could go wrong (plain Euler; the second evaluation at t[i])."""
import pytest
import torch

import f5_tts_amd as P
import ode_oracle as OO
from conftest import load_golden, synthetic_weights
from f5_tts_amd import _lib
from oracle import f5_oracle as O
from oracle import ref_harness as rh

FIXTURES = ["sample_b1_midpoint", "sample_b3_midpoint_attnmask", "sample_b1_midpoint_nocfg", "sample_unett_b2_midpoint"]
TOL_GPU = 1e-3   # the GPU parity bar these fixtures are held to (tests/test_ode_midpoint_gpu.py)


def _tiny_dit():
    return P.DiT(**P.config.F5TTS_TINY, text_num_embeds=40, mel_dim=100)


# ------------------------------------------------------------------------------------------------ public surface
def test_cfm_accepts_midpoint():
    m = P.CFM(transformer=_tiny_dit(), mel_spec_module=P.mel.MelSpec(), odeint_kwargs=dict(method="midpoint"))
    assert m.odeint_kwargs["method"] == "midpoint"
    P.CFM(transformer=_tiny_dit(), mel_spec_module=P.mel.MelSpec(), odeint_kwargs=dict(method="euler"))


def test_cfm_rejects_other_methods_and_names_the_supported_ones():
    with pytest.raises(NotImplementedError) as ei:
        P.CFM(transformer=_tiny_dit(), mel_spec_module=P.mel.MelSpec(), odeint_kwargs=dict(method="rk4"))
    assert "euler" in str(ei.value) and "midpoint" in str(ei.value)


def test_load_model_passes_ode_method_through():
    from f5_tts_amd import infer as I
    m = I.load_model(P.DiT, P.config.F5TTS_TINY, None, ode_method="midpoint", device="cpu")
    assert m.odeint_kwargs == dict(method="midpoint")


def test_abi_method_constants_and_unknown_method():
    assert (_lib.F5_ODE_EULER, _lib.F5_ODE_MIDPOINT) == (0, 1)
    assert _lib.ODE_METHODS == {"euler": 0, "midpoint": 1}
    lib = _lib.load()
    t = _lib.float_array([0.0, 1.0])
    rc = lib.f5_sample_ode(None, None, 0, None, None, None, 1, t, 1, 2.0, None, 1, 8, None, None, None, 7)
    assert rc == -1 and b"unknown ODE method 7" in lib.f5_last_error()
    rc = lib.f5_sample_ode(None, None, 0, None, None, None, 1, t, 1, 2.0, None, 1, 8, None, None, None, _lib.F5_ODE_MIDPOINT)
    assert rc == -1 and b"null engine" in lib.f5_last_error()


# ------------------------------------------------------------------------------------------------ the solver itself
def _grid(n=9):
    return O.time_grid(n - 1, -1.0, True)   # an EPSS + sway grid: uneven steps, as sample() uses


def test_euler_branch_is_the_oracles_euler_bit_for_bit():
    g = torch.Generator().manual_seed(3)
    y0 = torch.randn(2, 5, 7, generator=g)
    W = torch.randn(7, 7, generator=g) * 0.3

    def fn(t, y):
        return torch.tanh(y @ W) * torch.cos(3 * t) + y * t

    t = _grid(17)
    assert torch.equal(OO.fixed_grid_odeint(fn, y0, t, "euler"), O.euler_odeint(fn, y0, t))


def test_midpoint_is_exact_on_a_linear_in_time_field():
    """dy/dt = a + b t: the midpoint rule integrates it exactly (up to rounding); Euler does not."""
    a, b = 0.7, -2.3
    t = _grid(9).double()
    y0 = torch.tensor([0.25], dtype=torch.float64)
    exact = y0 + a * (t - t[0]) + 0.5 * b * (t * t - t[0] * t[0])

    def fn(tt, y):
        return torch.full_like(y, a) + b * tt

    mid = OO.fixed_grid_odeint(fn, y0, t, "midpoint")[:, 0]
    eul = OO.fixed_grid_odeint(fn, y0, t, "euler")[:, 0]
    assert (mid - exact).abs().max() < 1e-12
    assert (eul - exact).abs().max() > 1e-2
    assert (OO.fixed_grid_odeint(fn, y0, t, "midpoint", mid_at_half=False)[:, 0] - exact).abs().max() > 1e-2


def test_midpoint_step_factor_on_a_linear_field():
    """dy/dt = lam * y: every midpoint step multiplies y by 1 + lam dt + (lam dt)^2 / 2."""
    lam = -1.7
    t = _grid(9).double()
    y0 = torch.tensor([1.5, -0.5], dtype=torch.float64)
    ys = OO.fixed_grid_odeint(lambda tt, y: lam * y, y0, t, "midpoint")
    assert ys.shape == (t.shape[0], 2)
    for i in range(t.shape[0] - 1):
        h = lam * (t[i + 1] - t[i])
        assert torch.allclose(ys[i + 1], ys[i] * (1 + h + h * h / 2), rtol=1e-14, atol=0)


def test_midpoint_makes_two_evaluations_per_step_at_the_half_times():
    t = _grid(5)
    seen = []

    def fn(tt, y):
        seen.append(float(tt))
        return y

    traj = OO.fixed_grid_odeint(fn, torch.ones(3), t, "midpoint")
    assert traj.shape == (5, 3) and len(seen) == 8
    for i in range(4):
        half = 0.5 * (t[i + 1] - t[i])
        assert seen[2 * i] == float(t[i]) and seen[2 * i + 1] == float(t[i] + half)


def test_solver_context_swaps_and_restores_the_oracle_solver():
    saved = O.euler_odeint
    with OO.solver("midpoint"):
        assert O.euler_odeint is not saved
    assert O.euler_odeint is saved
    with pytest.raises(NotImplementedError):
        OO.fixed_grid_odeint(lambda t, y: y, torch.ones(1), _grid(3), "rk4")


# ------------------------------------------------------------------------------------------------ fixtures
def oracle_sample(meta, a, **solver_kw):
    """oracle.f5_oracle.sample on a fixture's problem (time-MLP factor applied) with the given solver."""
    sd = OO.scaled_time_mlp(synthetic_weights(meta), meta["time_mlp_scale"])
    dur = meta["duration"]
    dur = dur if isinstance(dur, int) else torch.tensor(dur)
    kw = dict(steps=meta["steps"], cfg_strength=meta["cfg_strength"], sway_sampling_coef=meta["sway"], seed=meta["seed"],
              use_epss=meta["use_epss"], no_ref_audio=meta["no_ref_audio"], backbone=meta["backbone"])
    if meta["lens"] is not None:
        kw["lens"] = torch.tensor(meta["lens"])
    if meta["duplicate_test"]:
        kw.update(duplicate_test=True, t_inter=meta["t_inter"])
    with OO.solver(**solver_kw):
        return O.sample(sd, meta["arch"], a["cond"], a["text"], dur, **kw)


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_midpoint_matches_fixture_and_wrong_solvers_do_not(name):
    meta, a = load_golden(name)
    assert meta["method"] == "midpoint" and meta["time_mlp_scale"] > 0
    out, traj = oracle_sample(meta, a, method="midpoint")
    assert traj.shape == a["traj"].shape and traj.shape[0] == int(meta["steps"] * (1 - meta["t_inter"] if meta["duplicate_test"] else 1)) + 1
    e = (traj - a["traj"]).abs().max().item()
    e_out = (out - a["out"]).abs().max().item()
    e_euler = (oracle_sample(meta, a, method="euler")[1] - a["traj"]).abs().max().item()
    e_wrong_t = (oracle_sample(meta, a, method="midpoint", mid_at_half=False)[1] - a["traj"]).abs().max().item()
    print(f"[oracle midpoint] {name}: traj Linf {e:.2e}; Euler {e_euler:.2e}; midpoint evaluated at t[i] {e_wrong_t:.2e}")
    assert e <= 2e-5 and e_out <= 2e-5
    assert e_euler >= 10 * TOL_GPU and e_wrong_t >= 10 * TOL_GPU


@pytest.mark.skipif(not rh.available(), reason="the reference tree is needed to regenerate the fixtures")
@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_regenerates_bit_identically_from_the_reference(name):
    import importlib.util
    import os

    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("make_golden_ode", os.path.join(ROOT, "tools", "make_golden_ode.py"))
    G = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(G)
    meta, arrays = G.generate(name)
    gmeta, a = load_golden(name)
    # (the checksum is a float64 sum whose last bits follow torch's host thread count: conftest.synthetic_weights' tolerance)
    chk, gchk = meta.pop("weights_checksum"), gmeta.pop("weights_checksum")
    assert abs(chk - gchk) <= 1e-6 * abs(gchk)
    assert meta == gmeta
    for k, v in arrays.items():
        assert torch.equal(v, a[k]), f"{name}: {k} differs from the committed fixture"
