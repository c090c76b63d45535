"""Inputs shared by tests/test_text_encoder.py (CPU) and tests/test_text_encoder_gpu.py: weights that make every term of
the text encoder count, the case table, and per case the float64 reference, the float32 CPU oracle and the error bound.

Weights.  weights.synthetic_state_dict draws grn.gamma, grn.beta and the pointwise weights from N(0, 0.02): the whole
ConvNeXt branch is then a perturbation of about 1e-3 on top of E[id] + pos, and a GRN that is wrong by 5 % moves the
output by 1e-4.  scaled_text_weights() overwrites the `text_embed.text_blocks.*` tensors (seeded per tensor name):
gamma ~ N(0, 0.7), beta ~ N(0, 0.3), pointwise weights ~ N(0, 1 / fan_in), every bias ~ N(0, 0.2), norm weights
uniform in 1 +- 0.3.  The depthwise taps (N(0, 0.3)) and the embedding table (N(0, 1)) keep their synthetic values.

Bound (per case and drop_text value): 8 x the L-inf error of the float32 CPU oracle against the float64 reference on the
same inputs, floored at 4 ulp of float32 at the output's largest magnitude.  The factor covers a different but equally
valid float32 summation order (64-lane wave reductions, 16 GRN partials, the GEMM's K blocking; sqrt(K)-ish growth).
"""
from __future__ import annotations

import functools
import math
import zlib
from dataclasses import dataclass, field

import torch

import f5_tts_amd as P
from oracle import f5_oracle as O
from text_oracle import text_embed64

NV = 40     # vocabulary: text ids 0 .. NV - 1, -1 is the filler; the embedding table has NV + 1 rows
BOUND_FACTOR = 8.0
FLOOR_ULPS = 4.0


def param_shapes(backbone, arch):
    if backbone == "DiT":
        return P.weights.dit_param_shapes(arch, NV)
    s = P.weights.unett_param_shapes(arch, NV)      # (lists no text blocks: E2-TTS has none; unett.py supports them)
    Dt = s["text_embed.text_embed.weight"][1]
    for i in range(arch.get("conv_layers", 0)):
        p = f"text_embed.text_blocks.{i}"
        s.update({p + ".dwconv.weight": (Dt, 1, 7), p + ".dwconv.bias": (Dt,), p + ".norm.weight": (Dt,),
                  p + ".norm.bias": (Dt,), p + ".pwconv1.weight": (2 * Dt, Dt), p + ".pwconv1.bias": (2 * Dt,),
                  p + ".grn.gamma": (1, 1, 2 * Dt), p + ".grn.beta": (1, 1, 2 * Dt), p + ".pwconv2.weight": (Dt, 2 * Dt),
                  p + ".pwconv2.bias": (Dt,)})
    return s


def scaled_text_weights(shapes, seed=0):
    sd = P.weights.synthetic_state_dict(shapes, seed=seed)
    for name, t in sd.items():
        if not name.startswith("text_embed.text_blocks.") or name.endswith(".dwconv.weight"):
            continue
        g = torch.Generator().manual_seed((zlib.crc32(name.encode()) ^ (0x7E47 + seed)) & 0x7FFFFFFF)
        if name.endswith(".norm.weight"):
            v = 0.7 + 0.6 * torch.rand(t.shape, generator=g)
        else:
            if name.endswith(".grn.gamma"):
                std = 0.7
            elif name.endswith(".grn.beta"):
                std = 0.3
            elif name.endswith(".bias"):
                std = 0.2
            else:                                   # pwconv1 / pwconv2 weight [out, in]: variance 1 / fan_in
                std = t.shape[1] ** -0.5
            v = torch.randn(t.shape, generator=g) * std
        sd[name] = v.to(torch.float32).contiguous()
    return sd


@dataclass(frozen=True)
class Case:
    name: str
    backbone: str
    text_dim: int | None        # None: the mel dimension, 100
    layers: int
    B: int
    N: int
    nt: int
    lens: tuple | None = None
    mask_padding: bool = True
    upsample: bool = False
    fillers: tuple = field(default=())      # (sample, first, last + 1): text positions overwritten with the filler
    note: str = ""

    @property
    def arch(self):
        a = dict(dim=256, depth=1 if self.backbone == "DiT" else 2, heads=4, dim_head=64, ff_mult=2, text_dim=self.text_dim,
                 conv_layers=self.layers, text_mask_padding=self.mask_padding, pe_attn_head=None, attn_mask_enabled=False,
                 qk_norm=None)
        if self.upsample:
            a["text_embedding_average_upsampling"] = True
        return a

    @property
    def key(self):
        """Cases with one key share weights (and, on the GPU, an engine)."""
        return (self.backbone, self.text_dim, self.layers, self.mask_padding, self.upsample)


LENS3 = (131, 37, 2)    # == N;  < N, not a multiple of 4 or 16;  below the 7 taps and the 16 GRN partials
CASES = [
    # ---- DiT
    Case("d64_l2_nomask", "DiT", 64, 2, 2, 50, 20, mask_padding=False, fillers=((0, 7, 9), (1, 14, 20)),
         note="the fixtures' shape; filler inside the text, rows not zeroed"),
    Case("d64_l2_mask", "DiT", 64, 2, 2, 50, 20, fillers=((0, 7, 9), (1, 14, 20)), note="same, filler rows zeroed"),
    Case("d64_l4_fillers", "DiT", 64, 4, 3, 131, 40, LENS3, fillers=((0, 5, 8), (0, 20, 21), (1, 0, 40)),
         note="filler inside sample 0, sample 1 all filler, lens 131 / 37 / 2"),
    Case("d100_l1_trunc", "DiT", None, 1, 2, 67, 80, (67, 5), mask_padding=False, fillers=((0, 30, 32),),
         note="nt > N; K = 100 / 200: the v1 GEMM; one block writes straight to out"),
    Case("d512_l4", "DiT", 512, 4, 3, 131, 40, LENS3, fillers=((0, 11, 13),), note="Base text dims"),
    Case("d512_l4_up", "DiT", 512, 4, 3, 131, 40, LENS3, upsample=True, fillers=((0, 11, 13),), note="same, average upsampling"),
    Case("d1024_l1", "DiT", 1024, 1, 1, 19, 12, note="4 of the 8 channel chunks; rows % 4 = 3"),
    Case("d2048_l1", "DiT", 2048, 1, 1, 19, 12, note="all 8 chunks: the widest text_dim f5_create accepts"),
    Case("d64_l0", "DiT", 64, 0, 2, 23, 10, (23, 9), note="no conv layers: the embedding alone, no position table"),
    # ---- average upsampling (text_dim 64, 2 layers, mask_padding on)
    Case("up_ratios", "DiT", 64, 2, 4, 48, 12, (48, 36, 12, 7), upsample=True, fillers=((3, 0, 2), (3, 3, 12)),
         note="valid tokens 12 / 12 / 12 / 1: rem 0 at base 4 and 3, tl == alen, tl == 1"),
    Case("up_rem2", "DiT", 64, 2, 2, 50, 12, upsample=True, fillers=((1, 4, 5),), note="50 % 12 = 2; 50 % 11 = 6"),
    Case("up_all_filler", "DiT", 64, 2, 2, 48, 12, (48, 30), upsample=True, fillers=((1, 0, 12),),
         note="sample 1 has no valid token (tl == 0): its rows are zero"),
    # ---- UNetT: embeds at the padded length whatever `lens` says; position row min(n, 4095)
    Case("u64_l2", "UNetT", 64, 2, 2, 50, 20, (50, 31), fillers=((0, 7, 9), (1, 14, 20)), note="lens given and ignored"),
    Case("u64_l1_clamp", "UNetT", 64, 1, 1, 4100, 40, mask_padding=False, note="rows 4095 .. 4099 use position row 4095"),
]
CASE = {c.name: c for c in CASES}
assert len(CASE) == len(CASES)


@functools.lru_cache(maxsize=None)
def weights_for(key):
    c = next(c for c in CASES if c.key == key)
    return scaled_text_weights(param_shapes(c.backbone, c.arch), seed=1)


def text_for(c: Case):
    g = torch.Generator().manual_seed(zlib.crc32(c.name.encode()) & 0x7FFFFFFF)
    text = torch.randint(0, NV, (c.B, c.nt), generator=g)
    for b, i0, i1 in c.fillers:
        text[b, i0:i1] = -1
    return text


@functools.lru_cache(maxsize=None)
def reference(name, drop_text, mutate=None):
    """float64 [B, N, Dt] (cached; callers must not write to it)."""
    c = CASE[name]
    return text_embed64(weights_for(c.key), P.config.normalize_arch(c.arch), text_for(c), c.N, c.lens, drop_text, c.backbone, mutate)


@functools.lru_cache(maxsize=None)
def oracle32(name, drop_text):
    """The project's float32 CPU oracle on the same inputs."""
    c = CASE[name]
    sd, arch, text = weights_for(c.key), P.config.normalize_arch(c.arch), text_for(c)
    if c.backbone == "UNetT":
        return O.unett_text_embed(sd, arch, text, c.N, drop_text)
    mask = None if c.lens is None else O.lens_to_mask(torch.tensor(c.lens), c.N)
    return O.text_embed_batch(sd, arch, text, c.N, mask, drop_text)


def ulp32(x: float) -> float:
    """Spacing of float32 at magnitude x (a normal number)."""
    return 2.0 ** (math.floor(math.log2(max(x, 2.0 ** -126))) - 23)


@functools.lru_cache(maxsize=None)
def bound(name, drop_text):
    """(bound, float32 oracle error, largest output magnitude)."""
    ref = reference(name, drop_text)
    e32 = (oracle32(name, drop_text).double() - ref).abs().max().item()
    top = ref.abs().max().item()
    return max(BOUND_FACTOR * e32, FLOOR_ULPS * ulp32(top)), e32, top
