"""Restatements for the isolated-rows tests (f5_set_isolated_rows): the two per-item ODE updates on PACKED rows as numpy float32
arithmetic, operation by operation in the kernels' order (no fused multiply-add: the library is built with -ffp-contract=off), the
4-row-rounded row table they index with, and the pitched staging of a slice."""
import numpy as np

F32 = np.float32


def row_start(lens, halves):
    """The RowPack table of `halves` x B batch rows (the conditional half, then the unconditional one): the first packed row of every
    batch row, each length rounded up to 4 rows, and the row count behind the last."""
    t = [0]
    for q in range(halves * len(lens)):
        t.append(t[-1] + -(-int(lens[q % len(lens)]) // 4) * 4)
    return np.array(t, np.int32)


def _update(y, pred, rs, lens, t_items, cfg, steps, step, use_cfg, half):
    """y [B, N, mel] after one update: pred [rows, mel] on packed rows, rs the 4-row-rounded row_start table (row_start()).  Item b
    with step < steps[b], frames n < lens[b]: v = p + (p - u) * cfg[b] (both halves ran and cfg[b] >= 1e-5) or p; Euler
    y + dt * v, the midpoint half step y + v * (0.5 * dt).  Everything else of y is returned as it was."""
    B = y.shape[0]
    out = y.astype(F32).copy()
    for b in range(B):
        if not step < steps[b]:
            continue
        n = int(lens[b])
        dt = F32(F32(t_items[b][step + 1]) - F32(t_items[b][step]))
        p = pred[rs[b]:rs[b] + n].astype(F32)
        v = p
        if use_cfg and not F32(cfg[b]) < F32(1e-5):
            u = pred[rs[B + b]:rs[B + b] + n].astype(F32)
            v = p + (p - u) * F32(cfg[b])
        out[b, :n] = y[b, :n] + v * F32(F32(0.5) * dt) if half else y[b, :n] + dt * v
    return out


def euler_items_packed(y, pred, rs, lens, t_items, cfg, steps, step, use_cfg):
    return _update(y, pred, rs, lens, t_items, cfg, steps, step, use_cfg, False)


def midpoint_half_items_packed(y, pred, rs, lens, t_items, cfg, steps, step, use_cfg):
    return _update(y, pred, rs, lens, t_items, cfg, steps, step, use_cfg, True)


def span_stage_pitched(y, prev, y_new, rows, N):
    """y [B, pitch, mel] with the frames n < N of every row staged -- prev[rows[b], n] (n < prev_N, else +0.0) where rows[b] >= 0,
    y_new[b, n] where rows[b] == -1 -- and every other frame as it was."""
    out = y.copy()
    for b, r in enumerate(rows):
        if r < 0:
            out[b, :N] = y_new[b]
        else:
            out[b, :N] = 0.0
            n = min(N, prev.shape[1])
            out[b, :n] = prev[r, :n]
    return out
