"""Inputs shared by tests/test_backbone_exposure.py (CPU), tests/test_backbone_float64_gpu.py and tools/make_exposed_golden.py:
weights on which every block of the DiT and the UNetT counts, the case table, the float64 reference and the wrong variants.

Weights.  On weights.synthetic_state_dict (N(0, 0.02)) the attention logits are near zero, the softmax is near uniform and the
AdaLN gates are about 0.06: one block without its rotary embedding moves a cfg_infer output by 1e-4, inside every gate of the
suite.  exposing_weights() multiplies tensors of that state dict by name and leaves the rest as generated:

    DiT     attn.to_q.weight, attn.to_k.weight x 10;  attn_norm.linear.weight, norm_out.linear.weight x 8;  ff.ff.0.0.weight x 3;
            q_norm.weight, k_norm.weight x 2 (qk_norm normalises the q / k factor away)
    UNetT   to_q.weight, to_k.weight x 6

The float64 reference is oracle/f5_oracle.py's own forward on double copies of the weights and inputs (forward64).  Two tables stay
what the reference makes them: the rotary angles and the sinus features of the time are float32 arithmetic there, so they are
computed in float32 and then widened (as tests/mmdit_oracle.py does).  For sample() the ODE state and the time grid are float32, as
the reference keeps them, around that forward (sample64).

Wrong variants (VARIANTS): each restates one operation of ONE block with one deliberate error -- the errors an engine that
composes its block stages wrongly would make: which rope table, pe_heads, q_scale, key count and AdaLN table slice a launch
receives.  A variant is applied only to the cases where it differs by definition (applies()).  `time_next_step` is the sample()
variant: step s is evaluated with step s + 1's time.

Seeds.  The factors above are fixed; the seeds are not, and one variant depends on them: "last key dropped" at B = 1, N = 65 removes one
key of 65 and moves the output by 5e-4 .. 7e-3 depending on the weights' and the inputs' seed (every other variant clears 4e-3 at
every seed tried).  WSEED = 3 and the input seed 20 of dit_options are the first pair of a scan (weights 0 .. 4, inputs 20 .. 27) at
which every block clears it with a tenth to spare; the float64 shifts are deterministic (MIN_SHIFT).

Not detectable by these tests (measured on the [65, 37] case, float64): exact GELU in place of the tanh form moves the output by
1.9e-5 and a LayerNorm eps of 1e-5 by 1.7e-5.  The FF1 epilogue is held to float64 in tests/test_epilogues_gpu.py.
"""
from __future__ import annotations

import contextlib
import functools
from dataclasses import dataclass, field

import torch
import torch.nn.functional as F

import f5_tts_amd as P
from oracle import f5_oracle as O

NV = 40               # text ids 0 .. NV - 1; -1 is the filler
TIME = 0.37
GATE_F32 = 2e-4       # the project's per-forward f32 gate (tests/test_sample_gpu.py, forward taps)
EXPOSED = 20 * GATE_F32   # what every wrong variant must move the output by: the factor tools/make_mmdit_golden.py uses
PLAIN_BAR = 1e-3      # the sample() parity bar: on the plain weights the logit variants of the DiT stay under it
NFE, CFG, SWAY, SEED = 4, 2.0, -1.0, 7
WSEED = 3            # seed of the synthetic weights (see "Seeds" in the header)

FACTORS = {
    "DiT": ((("attn.to_q.weight", "attn.to_k.weight"), 10.0), (("attn_norm.linear.weight", "norm_out.linear.weight"), 8.0),
            (("ff.ff.0.0.weight",), 3.0), (("q_norm.weight", "k_norm.weight"), 2.0)),
    "UNetT": (((".2.to_q.weight", ".2.to_k.weight"), 6.0),),
}

DIT_TINY = dict(dim=256, depth=4, heads=4, dim_head=64, ff_mult=2, text_dim=64, conv_layers=2, text_mask_padding=False,
                pe_attn_head=None, attn_mask_enabled=False, qk_norm=None)
UNETT_TINY = dict(dim=256, depth=4, heads=4, dim_head=64, ff_mult=2, text_dim=None, conv_layers=0, text_mask_padding=False,
                  pe_attn_head=None, attn_mask_enabled=False, qk_norm=None)


def param_shapes(backbone, arch, nv=NV):
    return (P.weights.dit_param_shapes if backbone == "DiT" else P.weights.unett_param_shapes)(arch, nv)


def exposing_weights(backbone, arch, nv=NV, seed=0):
    sd = P.weights.synthetic_state_dict(param_shapes(backbone, arch, nv), seed=seed)
    for name in sd:
        for suffixes, factor in FACTORS[backbone]:
            if name.endswith(suffixes):
                sd[name] = (sd[name] * factor).contiguous()
    return sd


def weights_checksum(sd):
    return float(sum(v.double().abs().sum().item() for v in sd.values()))


@dataclass(frozen=True)
class Case:
    name: str
    backbone: str
    B: int
    N: int
    lens: tuple | None
    over: tuple = field(default=())     # arch keys that differ from the backbone's tiny arch
    seed: int = 0
    note: str = ""

    @property
    def arch(self):
        return dict(DIT_TINY if self.backbone == "DiT" else UNETT_TINY, **dict(self.over))

    @property
    def key(self):
        """Cases with one key share weights (and, on the GPU, an engine)."""
        return (self.backbone, self.over)


CASES = [
    Case("dit_packed", "DiT", 3, 129, (129, 17, 65), (("attn_mask_enabled", True),), 11,
         "packed rows; crosses a 128-row GEMM tile and a 64-key attention tile; rotary on every head"),
    Case("dit_padded", "DiT", 3, 129, (129, 17, 65), (("pe_attn_head", 1),), 12, "rectangular rows, pad keys attended; rotary on head 0"),
    Case("dit_options", "DiT", 1, 65, None, (("qk_norm", "rms_norm"), ("long_skip_connection", True)), 20, "B = 1, no mask"),
    Case("dit_b2", "DiT", 2, 65, (65, 37), (("attn_mask_enabled", True),), 14, "packed; the case of the reference-generated fixture"),
    Case("unett_masked", "UNetT", 2, 65, (65, 37), (("attn_mask_enabled", True),), 15, "N + 1 rows, the time token at rotary position 0"),
    Case("unett_b2", "UNetT", 2, 65, (65, 37), (), 16, "the same, pad keys attended; the case of the reference-generated fixture"),
]
CASE = {c.name: c for c in CASES}
assert len(CASE) == len(CASES)
FORWARD_CASES = [c.name for c in CASES]
SAMPLE_CASES = {"DiT": "dit_b2", "UNetT": "unett_b2"}
NT = 20               # text columns: longer than the 17-frame item (truncated there), shorter than the others


@functools.lru_cache(maxsize=None)
def weights_for(key, plain=False):
    c = next(c for c in CASES if c.key == key)
    if plain:
        return P.weights.synthetic_state_dict(param_shapes(c.backbone, c.arch), seed=WSEED)
    return exposing_weights(c.backbone, c.arch, NV, seed=WSEED)


def cfg_of(c: Case):
    return P.config.normalize_arch(c.arch)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(x, cond, text, time, mask): x and cond ~ N(0, 1) on every frame, valid text of 9 .. NT tokens per item."""
    c = CASE[name]
    g = torch.Generator().manual_seed(5000 + c.seed)
    x = torch.randn(c.B, c.N, 100, generator=g)
    cond = torch.randn(c.B, c.N, 100, generator=g)
    text = torch.randint(0, NV, (c.B, NT), generator=g)
    for b in range(1, c.B):
        text[b, NT - 4 * b:] = -1
    mask = None if c.lens is None else O.lens_to_mask(torch.tensor(c.lens), c.N)
    return x, cond, text, torch.tensor(TIME), mask


def valid(name, halves=2):
    """bool[halves * B, N, 1]: the frames inside each item's own length."""
    c = CASE[name]
    lens = torch.tensor(c.lens if c.lens is not None else [c.N] * c.B)
    return (torch.arange(c.N)[None, :] < lens[:, None])[..., None].repeat(halves, 1, 1)


def linf(a, b, v=None):
    d = (a.double() - b.double()).abs()
    return (d if v is None else d * v).max().item()


# ------------------------------------------------------------------------------------------- the float64 reference
@contextlib.contextmanager
def _patched(**attrs):
    saved = {k: getattr(O, k) for k in attrs}
    for k, v in attrs.items():
        setattr(O, k, v)
    try:
        yield
    finally:
        for k, v in saved.items():
            setattr(O, k, v)


_rotary_freqs, _sinus_features = O.rotary_freqs, O.sinus_features


def _float64_tables():
    """The two tables the reference computes in float32 whatever the model's dtype: float32 arithmetic, then widened."""
    return _patched(rotary_freqs=lambda n, dim_head, base=10000.0: _rotary_freqs(n, dim_head, base).double(),
                    sinus_features=lambda t, dim=256, scale=1000.0: _sinus_features(t.float(), dim, scale).double())


_W64: dict = {}


def _double(W):
    key = id(W)
    if key not in _W64 or _W64[key][0] is not W:
        _W64[key] = (W, {k: v.double() for k, v in W.items()})
    return _W64[key][1]


_FORWARD = {"DiT": O.dit_forward, "UNetT": O.unett_forward}


def forward64(backbone, W, cfg, x, cond, text, time, mask=None, drop_audio_cond=False, drop_text=False, cfg_infer=False, cache=None,
              wrong=None):
    """One backbone call of the oracle in float64 (weights, activations, softmax), returned in float64.  wrong = (variant, block)
    applies one wrong variant to one block."""
    with _float64_tables(), (wrong_block(*wrong) if wrong else contextlib.nullcontext()):
        return _FORWARD[backbone](_double(W), cfg, x.double(), cond.double(), text, time.double(), mask, drop_audio_cond, drop_text,
                                  cfg_infer, cache)


@functools.lru_cache(maxsize=None)
def reference(name, plain=False):
    """float64 [2 B, N, mel]: the cfg_infer forward of a case (cached; callers must not write to it)."""
    c = CASE[name]
    return forward64(c.backbone, weights_for(c.key, plain), cfg_of(c), *inputs(name), cfg_infer=True)


@functools.lru_cache(maxsize=None)
def oracle32(name):
    """The project's float32 CPU oracle on the same inputs."""
    c = CASE[name]
    return _FORWARD[c.backbone](weights_for(c.key), cfg_of(c), *inputs(name), cfg_infer=True)


def oracle32_error(name):
    return linf(oracle32(name), reference(name), valid(name))


# ------------------------------------------------------------------------------------------------ wrong variants
LOGIT_VARIANTS = ("no_rotary", "pe_heads", "q_scale_halved", "q_one_off", "last_key_dropped")
VARIANTS = {
    "no_rotary": "no rotary embedding",
    "pe_heads": "rotary on head 0 only where every head has it, on every head where only head 0 has it",
    "q_scale_halved": "q.k scale halved (with qk_norm: q_norm.weight halved)",
    "q_one_off": "q rotated one position off k",
    "last_key_dropped": "the last valid key of every item dropped",
    "key_mask_flipped": "key mask ignored; where attn_mask_enabled is off, pad keys masked although the option is off",
    "v_heads_swapped": "v heads 0 and 1 swapped",
    "gates_swapped": "msa and mlp gates swapped",
    "block_skipped": "block skipped (UNetT: its attention and feed-forward)",
    "adaln_next_block": "block i modulated with block i + 1's AdaLN vectors (the last block: with block i - 1's)",
}


def applies(variant, c: Case):
    if variant in ("gates_swapped", "adaln_next_block"):
        return c.backbone == "DiT"
    if variant == "key_mask_flipped":
        return c.lens is not None and min(c.lens) < c.N
    return True


def variants_of(c: Case):
    return [v for v in VARIANTS if applies(v, c)]


def _attention(W, cfg, pfx, x, mask, freqs, v=None):
    """O.attention with the deliberate error v; v None is O.attention operation for operation (the CPU test checks it bit for bit)."""
    b, n, _ = x.shape
    H, dh = cfg["heads"], cfg.get("dim_head", 64)
    q, k, val = (O.linear(x, W, f"{pfx}.{m}").view(b, n, H, dh).transpose(1, 2) for m in ("to_q", "to_k", "to_v"))
    scale = dh ** -0.5
    if cfg.get("qk_norm") is not None:
        gq = W[pfx + ".q_norm.weight"] * (0.5 if v == "q_scale_halved" else 1.0)
        q = F.rms_norm(q, (dh,), weight=gq, eps=1e-6)
        k = F.rms_norm(k, (dh,), weight=W[pfx + ".k_norm.weight"], eps=1e-6)
    elif v == "q_scale_halved":
        scale = 0.5 * scale
    if v == "v_heads_swapped":
        val = torch.cat((val[:, 1:2], val[:, 0:1], val[:, 2:]), dim=1)
    pn = cfg.get("pe_attn_head")
    if v == "pe_heads":
        pn = 1 if pn is None else None
    fq = O.rotary_freqs(n + 1, dh).to(freqs.dtype)[1:] if v == "q_one_off" else freqs
    if v != "no_rotary":
        if pn is None:
            q, k = O.rotary_apply(q, fq), O.rotary_apply(k, freqs)
        else:
            q = torch.cat((O.rotary_apply(q[:, :pn], fq), q[:, pn:]), dim=1)
            k = torch.cat((O.rotary_apply(k[:, :pn], freqs), k[:, pn:]), dim=1)
    s = torch.matmul(q, k.transpose(-1, -2)) * scale
    keys = mask if (cfg.get("attn_mask_enabled", False) and mask is not None) else None
    if v == "key_mask_flipped":
        keys = mask if keys is None else None
    if v == "last_key_dropped":
        keys = (torch.ones(b, n, dtype=torch.bool) if keys is None else keys).clone()
        keys[torch.arange(b), keys.sum(dim=1) - 1] = False
    if keys is not None:
        s = s.masked_fill(~keys[:, None, None, :], float("-inf"))
    o = torch.matmul(torch.softmax(s, dim=-1), val)
    o = o.transpose(1, 2).reshape(b, n, H * dh)
    o = O.linear(o, W, pfx + ".to_out.0")
    if mask is not None:
        o = o.masked_fill(~mask.unsqueeze(-1), 0.0)
    return o


def _dit_block(W, cfg, i, x, t, mask, freqs, v=None):
    """O.dit_block with the deliberate error v."""
    pfx = f"transformer_blocks.{i}"
    dim = x.shape[-1]
    src = i if v != "adaln_next_block" else (i + 1 if i + 1 < cfg["depth"] else i - 1)
    emb = O.linear(F.silu(t), W, f"transformer_blocks.{src}.attn_norm.linear")
    shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp = torch.chunk(emb, 6, dim=1)
    if v == "gates_swapped":
        gate_msa, gate_mlp = gate_mlp, gate_msa
    h = F.layer_norm(x, (dim,), eps=1e-6) * (1 + scale_msa[:, None]) + shift_msa[:, None]
    x = x + gate_msa.unsqueeze(1) * O.attention(W, cfg, pfx + ".attn", h, mask, freqs)
    h = F.layer_norm(x, (dim,), eps=1e-6) * (1 + scale_mlp[:, None]) + shift_mlp[:, None]
    h = F.gelu(O.linear(h, W, pfx + ".ff.ff.0.0"), approximate="tanh")
    h = O.linear(h, W, pfx + ".ff.ff.2")
    return x + gate_mlp.unsqueeze(1) * h


def wrong_block(variant, block):
    """Within the block, the oracle's forwards compute block `block` with the wrong variant `variant`."""
    assert variant in VARIANTS
    attention, dit_block, linear = O.attention, O.dit_block, O.linear
    mine = (f"transformer_blocks.{block}.attn", f"layers.{block}.2")
    patch = {}
    if variant == "block_skipped":
        patch["dit_block"] = lambda W, cfg, i, x, t, mask, freqs: x if i == block else dit_block(W, cfg, i, x, t, mask, freqs)
        patch["attention"] = lambda W, cfg, pfx, x, mask, freqs: (torch.zeros_like(x) if pfx == mine[1]
                                                                  else attention(W, cfg, pfx, x, mask, freqs))
        patch["linear"] = lambda x, W, name: (torch.zeros_like(linear(x, W, name)) if name == f"layers.{block}.4.ff.2"
                                              else linear(x, W, name))
    elif variant in ("gates_swapped", "adaln_next_block"):
        patch["dit_block"] = lambda W, cfg, i, x, t, mask, freqs: (_dit_block(W, cfg, i, x, t, mask, freqs, variant) if i == block
                                                                   else dit_block(W, cfg, i, x, t, mask, freqs))
    else:
        patch["attention"] = lambda W, cfg, pfx, x, mask, freqs: (_attention(W, cfg, pfx, x, mask, freqs, variant) if pfx in mine
                                                                  else attention(W, cfg, pfx, x, mask, freqs))
    return _patched(**patch)


def shift(name, variant, block, plain=False):
    """L-inf, on valid frames, by which the wrong variant in one block moves the float64 cfg_infer output of a case."""
    c = CASE[name]
    out = forward64(c.backbone, weights_for(c.key, plain), cfg_of(c), *inputs(name), cfg_infer=True, wrong=(variant, block))
    return linf(out, reference(name, plain), valid(name))


@functools.lru_cache(maxsize=None)
def shift_table(name, plain=False, variants=None):
    """{(variant, block): shift} of a case (cached)."""
    c = CASE[name]
    return {(v, i): shift(name, v, i, plain) for v in (variants or variants_of(c)) for i in range(c.arch["depth"])}


# Smallest shift per case over every block and applicable variant, measured with shift_table() in float64 on the CPU and rounded
# down; tests/test_backbone_exposure.py holds the table to these, the GPU test divides them by its gates.
MIN_SHIFT = {"dit_packed": 6.5e-3, "dit_padded": 7.5e-3, "dit_options": 4.5e-3, "dit_b2": 5.7e-3, "unett_masked": 7.2e-2, "unett_b2": 6.6e-2}


# --------------------------------------------------------------------------------------------------------- sample()
@functools.lru_cache(maxsize=None)
def sample_inputs(backbone):
    """(cond, text, duration, lens) of the backbone's sample() case: the forward case's lengths as durations, 24 and 16 prompt frames."""
    c = CASE[SAMPLE_CASES[backbone]]
    g = torch.Generator().manual_seed(7000 + c.seed)
    cond = torch.randn(c.B, 24, 100, generator=g)
    cond[1, 16:] = 0
    text = inputs(c.name)[2]
    return cond, text, torch.tensor(c.lens), torch.tensor([24, 16])


def sample_kwargs():
    return dict(steps=NFE, cfg_strength=CFG, sway_sampling_coef=SWAY, seed=SEED)


def sample64(backbone, method="euler", time_next_step=None, plain=False):
    """oracle.f5_oracle.sample (float32 ODE state and grid, the solver of tests/ode_oracle.py) around forward64, which hands its
    result back in the state's dtype.  time_next_step = s: the wrong variant that evaluates step s at step s + 1's time (Euler)."""
    import ode_oracle as OO

    c = CASE[SAMPLE_CASES[backbone]]
    W = weights_for(c.key, plain)
    cond, text, dur, lens = sample_inputs(backbone)
    grid = O.time_grid(NFE, SWAY)
    calls = [0]

    def fwd(W_, cfg, x, cond_, text_, time, mask=None, drop_audio_cond=False, drop_text=False, cfg_infer=False, cache=None):
        s = calls[0]
        calls[0] += 1
        if time_next_step is not None and s == time_next_step:
            assert method == "euler" and torch.equal(time, grid[s])
            time = grid[s + 1]
        return forward64(backbone, W_, cfg, x, cond_, text_, time, mask, drop_audio_cond, drop_text, cfg_infer, cache).to(x.dtype)

    with OO.solver(method), _patched(dit_forward=fwd, unett_forward=fwd):
        return O.sample(W, cfg_of(c), cond, text, dur, lens=lens, backbone=backbone, **sample_kwargs())


def sample_valid(backbone):
    """bool[B, N, 1] over the frames of each item's duration."""
    return valid(SAMPLE_CASES[backbone], halves=1)
