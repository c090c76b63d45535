"""Restatements for the per-item sampler tests (f5_sample_items): the time rows of a call, and the two ODE updates and the row gather
as numpy float32 arithmetic, operation by operation (no fused multiply-add: the library is built with -ffp-contract=off)."""
import ctypes as C

import numpy as np

F32 = np.float32


def item_time_rows(grids, steps, method):
    """(times, idx): the evaluation times of every live item, walked evaluation-major and then item-major, deduplicated by bit
    pattern in first-appearance order; idx[ev][b] is the row of item b's time at evaluation ev (0 once it has finished).
    grids: one list of f32 values per item, at least steps[b] + 1 long."""
    evals = 2 if method == "midpoint" else 1
    smax, B = max(steps), len(steps)
    times, rows, idx = [], {}, [[0] * B for _ in range(evals * smax)]
    for ev in range(evals * smax):
        i = ev // evals
        for b in range(B):
            if i >= steps[b]:
                continue
            t = F32(grids[b][i])
            if ev % evals:
                t = F32(t + F32(F32(0.5) * F32(F32(grids[b][i + 1]) - t)))
            key = t.tobytes()
            if key not in rows:
                rows[key] = len(times)
                times.append(t)
            idx[ev][b] = rows[key]
    return np.array(times, F32), np.array(idx, np.int32)


def k_item_time_rows(lib, grids, steps, method_id):
    """f5k_item_time_rows on host lists (no GPU needed): (rc, times[:U], idx[evals * steps_max][B])."""
    B, smax = len(steps), max(steps)
    evals = 2 if method_id == 1 else 1
    flat = []
    for g in grids:
        flat += [float(v) for v in g[:smax + 1]] + [0.0] * max(0, smax + 1 - len(g))
    times = (C.c_float * (evals * smax * B))()
    idx = (C.c_int32 * (evals * smax * B))()
    U = C.c_int32(-1)
    rc = lib.f5k_item_time_rows((C.c_float * len(flat))(*flat), (C.c_int32 * B)(*steps), smax, B, method_id, times, idx, C.byref(U))
    if rc != 0:
        return rc, None, None
    return rc, np.array(times[:U.value], F32), np.array(idx[:], np.int32).reshape(evals * smax, B)


def velocity(pred, cfg, use_cfg):
    """v [B, N, mel] of pred [halves, B, N, mel]: p + (p - u) * cfg for an item with cfg >= 1e-5 when both halves ran, else p."""
    p = pred[0].astype(F32)
    v = p.copy()
    if use_cfg:
        u = pred[1].astype(F32)
        for b, c in enumerate(cfg):
            if not F32(c) < F32(1e-5):
                v[b] = p[b] + (p[b] - u[b]) * F32(c)
    return v


def euler_items(y, pred, t_items, cfg, steps, step, use_cfg):
    """y after the update of `step`: y + dt_b * v for the live items (step < steps[b]), y itself for the others."""
    v, out = velocity(pred, cfg, use_cfg), y.astype(F32).copy()
    for b in range(y.shape[0]):
        if step < steps[b]:
            dt = F32(F32(t_items[b][step + 1]) - F32(t_items[b][step]))
            out[b] = y[b] + dt * v[b]
    return out


def midpoint_half_items(y, pred, t_items, cfg, steps, step, use_cfg):
    """y_mid: y + v * (dt_b / 2) for the live items, y for the others."""
    v, out = velocity(pred, cfg, use_cfg), y.astype(F32).copy()
    for b in range(y.shape[0]):
        if step < steps[b]:
            hdt = F32(F32(0.5) * F32(F32(t_items[b][step + 1]) - F32(t_items[b][step])))
            out[b] = y[b] + v[b] * hdt
    return out


def mod_gather(src, idx, rows):
    """dst[r] = src[idx[r % len(idx)]]"""
    return np.stack([src[idx[r % len(idx)]] for r in range(rows)])
