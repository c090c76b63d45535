"""Float64 restatement of CFM.forward's glue (the reference's cfm.py:261-302) around the in-repo oracle's backbone forward
(oracle/f5_oracle.py for the DiT and the UNetT, tests/mmdit_oracle.py for the MMDiT), with every draw an argument:

    phi  = (1 - t) x0 + t x1                                  per row, t = time[b]
    cond = x1 with the frames of span[b] = [start, end) zeroed
    pred = backbone(phi, cond, text, time, drop_audio_cond, drop_text, mask = lens_to_mask(lens))
    loss = mean over the span frames of all rows and over mel of (pred - (x1 - x0))^2

Weights, activations and sums are float64; the sinus time features are float32 arithmetic, as in the reference.  `variant` selects a
deliberately wrong glue that the fixtures must be able to tell from the right one:

    "span_shift"    the span one frame later (one frame earlier where it ends at the item's length)
    "time_roll"     every row evaluated at the time of the row before it
    "ignore_drops"  drop_audio_cond and drop_text ignored
    "whole_row"     the loss taken over every frame of the item, not over the span
"""
from __future__ import annotations

import contextlib

import torch

import f5_tts_amd as P
import mmdit_oracle
import ode_oracle
from oracle import f5_oracle as O

VARIANTS = ("span_shift", "time_roll", "ignore_drops", "whole_row")


def fixture_weights(meta):
    """The f32 state dict a flow-loss fixture was generated with: synthetic weights at the recorded std, the time MLP scaled."""
    shapes = {"DiT": P.weights.dit_param_shapes, "UNetT": P.weights.unett_param_shapes,
              "MMDiT": P.weights.mmdit_param_shapes}[meta["backbone"]](meta["arch"], meta["nvocab"])
    kw = dict(std=meta["std"]) if "std" in meta else {}
    sd = P.weights.synthetic_state_dict(shapes, seed=meta["wseed"], **kw)
    chk = float(sum(v.double().abs().sum().item() for v in sd.values()))
    assert abs(chk - meta["weights_checksum"]) <= 1e-6 * abs(chk), "synthetic weight generator drifted from the fixtures"
    return ode_oracle.scaled_time_mlp(sd, meta["time_mlp_scale"])


@contextlib.contextmanager
def _f32_time_features():
    saved = O.sinus_features
    O.sinus_features = lambda t, *a, **k: saved(t.float(), *a, **k).double()
    try:
        yield
    finally:
        O.sinus_features = saved


def backbone_forward(backbone, W, cfg, x, cond, text, time, mask, drop_audio_cond, drop_text):
    """One forward in float64 on the f32 weights W; x, cond float64, time float64 [B]."""
    if backbone == "MMDiT":
        return mmdit_oracle.forward(W, cfg, x, cond, text, time, mask=mask, drop_audio_cond=drop_audio_cond, drop_text=drop_text)
    W64 = {k: v.double() for k, v in W.items()}
    fn = O.dit_forward if backbone == "DiT" else O.unett_forward
    with _f32_time_features():
        return fn(W64, cfg, x, cond, text, time, mask=mask, drop_audio_cond=drop_audio_cond, drop_text=drop_text)


def flow_loss(backbone, W, cfg, x1, x0, text, time, span, lens, drop_audio_cond=False, drop_text=False, variant=None):
    """Returns a dict: loss (float64 scalar), sq_sum [B], count [B], per_item [B], pred, cond [B, N, mel], frame_err [B, N], all
    float64 (count: long)."""
    assert variant is None or variant in VARIANTS
    B, N, mel = x1.shape
    x1, x0, time = x1.double(), x0.double(), torch.as_tensor(time).double()
    lens = torch.as_tensor(lens)
    span = [tuple(int(v) for v in se) for se in span]
    if variant == "span_shift":
        span = [(s + 1, e + 1) if e < int(n) else (max(s - 1, 0), e - 1) for (s, e), n in zip(span, lens)]
    if variant == "time_roll":
        time = time.roll(1)
    if variant == "ignore_drops":
        drop_audio_cond = drop_text = False
    seq = torch.arange(N)
    in_span = torch.stack([(seq >= s) & (seq < e) for s, e in span])
    t = time[:, None, None]
    phi = (1 - t) * x0 + t * x1
    cond = torch.where(in_span[..., None], torch.zeros_like(x1), x1)
    mask = O.lens_to_mask(lens, N)
    pred = backbone_forward(backbone, W, cfg, phi, cond, text, time, mask, drop_audio_cond, drop_text).double()
    err = (pred - (x1 - x0)) ** 2
    sel = mask if variant == "whole_row" else in_span
    frame_err = torch.where(sel, err.mean(-1), torch.zeros(()).double())
    sq_sum = torch.where(sel[..., None], err, torch.zeros(()).double()).sum((1, 2))
    count = sel.sum(1)
    return dict(loss=sq_sum.sum() / (count.sum() * mel), sq_sum=sq_sum, count=count, per_item=sq_sum / (count * mel), pred=pred, cond=cond,
                frame_err=frame_err)


def loss_tolerance(loss_ref: float, e: float, n_selected: int) -> float:
    """How far a loss may lie from the reference's when its prediction lies within e (max abs) of the reference's:
    |mean((p + d - f)^2) - mean((p - f)^2)| = |mean(2 d (p - f) + d^2)| <= 2 e mean|p - f| + e^2 <= 2 e sqrt(loss_ref) + e^2
    (Cauchy-Schwarz), plus the worst case of the reference's own f32 mean over n_selected terms, loss_ref * n * 2^-24."""
    return 2.0 * loss_ref ** 0.5 * e + e * e + loss_ref * n_selected * 2.0 ** -24
