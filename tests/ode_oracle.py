"""Test-side fixed-grid ODE solvers: torchdiffeq's `odeint(fn, y0, t, method=...)` for method "euler" and "midpoint".

torchdiffeq is third-party and not installed; the rules are restated from its published solvers
(FixedGridODESolver.integrate with the grid `t` itself, Euler._step_func, Midpoint._step_func), all in the dtype of
`t` and `y0`, in this order:

    euler:     y = y + dt * fn(t[i], y)
    midpoint:  half = 0.5 * dt;  f0 = fn(t[i], y);  y_mid = y + f0 * half;  y = y + dt * fn(t[i] + half, y_mid)

with dt = t[i+1] - t[i].  The trajectory holds the grid points t[0..S] only.  The Euler branch is
oracle.f5_oracle.euler_odeint operation for operation (tests/test_ode_midpoint.py checks it bit for bit).

`solver(method)` runs oracle.f5_oracle.sample with one of these solvers; `scaled_time_mlp` applies the fixture's
time-MLP weight factor (meta["time_mlp_scale"]).
"""
from __future__ import annotations

import contextlib

import torch

METHODS = ("euler", "midpoint")
TIME_MLP_KEYS = ("time_embed.time_mlp.0.weight", "time_embed.time_mlp.2.weight")


def fixed_grid_odeint(fn, y0, t, method="euler", *, mid_at_half=True):
    """`mid_at_half=False` is a deliberately wrong midpoint (the second evaluation at t[i] instead of t[i] + half) that the
    fixtures must be able to tell apart from the right one."""
    if method not in METHODS:
        raise NotImplementedError(f"fixed-grid method {method!r}: expected one of {METHODS}")
    ys = [y0]
    y = y0
    for i in range(t.shape[0] - 1):
        if method == "euler":
            y = y + (t[i + 1] - t[i]) * fn(t[i], y)
        else:
            dt = t[i + 1] - t[i]
            half = 0.5 * dt
            f0 = fn(t[i], y)
            y_mid = y + f0 * half
            y = y + dt * fn(t[i] + half if mid_at_half else t[i], y_mid)
        ys.append(y)
    return torch.stack(ys, 0)


def reference_odeint(fn, y0, t, method="euler", **_kw):
    """Drop-in for `torchdiffeq.odeint` as the reference's cfm.py calls it (`odeint(fn, y0, t, **odeint_kwargs)`)."""
    return fixed_grid_odeint(fn, y0, t, method)


@contextlib.contextmanager
def solver(method="euler", *, mid_at_half=True):
    """Within the block, oracle.f5_oracle.sample integrates with `method` instead of its built-in Euler."""
    from oracle import f5_oracle as O

    saved = O.euler_odeint
    O.euler_odeint = lambda fn, y0, t: fixed_grid_odeint(fn, y0, t, method, mid_at_half=mid_at_half)
    try:
        yield
    finally:
        O.euler_odeint = saved


def scaled_time_mlp(sd: dict, factor: float) -> dict:
    """A copy of the state dict with both time-MLP weight matrices multiplied by `factor` (1.0: unchanged)."""
    if factor == 1.0:
        return sd
    return {k: (v * factor if k in TIME_MLP_KEYS else v) for k, v in sd.items()}
