"""Host side of the resident LoRA adapters (include/f5_hip.h, F5_OPT_ADAPTERS): which tensors an adapter may touch, the
scale of a low-rank pair, splitting a PEFT checkpoint into (base state dict, adapter tensors) and the two host merges --
torch's `B @ A` (the reference's arithmetic, infer/utils_infer.py:198-239) and the engine's contract rule, which the
device reproduces bit for bit.  Pure torch on the CPU; nothing here needs the library.

The fine-tunes this serves are made by the reference's train/train_lora.py: rank 16 (alpha 32) on to_q / to_k / to_v /
to_out.0 of every DiT block, rank 64 (alpha 128) on input_embed.proj, the text encoder (`text_embed.*`) trained in full.

Adapter tensors use plain names: `<module>.lora_A.weight` [r, in], `<module>.lora_B.weight` [out, r], and full
replacement tensors under their own state-dict names.
"""
from __future__ import annotations

import re

import torch

LORA_MODULE_RE = re.compile(r"^(transformer_blocks\.\d+\.attn\.(to_q|to_k|to_v|to_out\.0)|input_embed\.proj)$")
FULL_PREFIX = "text_embed."
MAX_RANK = 128
PEFT_PREFIX = "base_model.model."


def is_lora_module(module: str) -> bool:
    return LORA_MODULE_RE.match(module) is not None


def is_replaceable(name: str) -> bool:
    return name.startswith(FULL_PREFIX)


def _pattern_value(pattern: dict | None, module: str, default):
    """PEFT's rank_pattern / alpha_pattern lookup: a key matches a module whose name is the key or ends in `.key`
    (the key is a regular expression); the first matching key wins."""
    for key, val in (pattern or {}).items():
        if re.match(rf"(.*\.)?({key})$", module):
            return val
    return default


def pair_scale(module: str, lora_alpha=32, lora_r=16, alpha_pattern=None, rank_pattern=None) -> float:
    """alpha / r of one module with PEFT's per-module overrides (the reference's recipe: 32 / 16, and 128 / 64 for
    input_embed.proj)."""
    return float(_pattern_value(alpha_pattern, module, lora_alpha)) / float(_pattern_value(rank_pattern, module, lora_r))


def split_adapter_tensors(tensors: dict) -> tuple[dict, dict]:
    """Adapter tensors -> ({module: (A, B)}, {name: replacement tensor}), names and pairing checked."""
    pairs, full = {}, {}
    for k, v in tensors.items():
        m = re.match(r"^(.*)\.lora_([AB])\.weight$", k)
        if m is None:
            if not is_replaceable(k):
                raise ValueError(f"adapter tensor {k!r} is neither a LoRA pair nor replaceable in full (only {FULL_PREFIX}* is)")
            full[k] = v
            continue
        mod = m.group(1)
        if not is_lora_module(mod):
            raise ValueError(f"{mod!r} does not take a low-rank pair (adaptable: to_q / to_k / to_v / to_out.0 of every "
                             "DiT block and input_embed.proj)")
        pairs.setdefault(mod, [None, None])[0 if m.group(2) == "A" else 1] = v
    for mod, (a, b) in pairs.items():
        if a is None or b is None:
            raise ValueError(f"{mod}: lora_A and lora_B must both be given")
        if a.dim() != 2 or b.dim() != 2 or a.shape[0] != b.shape[1] or not 1 <= a.shape[0] <= MAX_RANK:
            raise ValueError(f"{mod}: lora_A {tuple(a.shape)} / lora_B {tuple(b.shape)} are not a pair of rank 1 .. {MAX_RANK}")
    return {m: (a, b) for m, (a, b) in pairs.items()}, full


def _strip(sd: dict) -> dict:
    """`ema_model.` / `base_model.model.` / `transformer.` prefixes off, bookkeeping and mel buffers dropped."""
    out = {}
    for k, v in sd.items():
        if k.startswith("ema_model."):
            k = k[len("ema_model."):]
        if k in ("initted", "step"):
            continue
        if k.startswith(PEFT_PREFIX):
            k = k[len(PEFT_PREFIX):]
        if k.startswith("mel_spec."):
            continue
        if k.startswith("transformer."):
            k = k[len("transformer."):]
        out[k] = v
    return out


def split_peft_state_dict(state_dict: dict, base: dict | None = None) -> tuple[dict, dict]:
    """A PEFT checkpoint's state dict (`base_model.model.*`, `.base_layer.`, `.lora_A/B.default.`; optional
    `ema_model.` / `transformer.` prefixes) -> (base state dict under plain names, adapter tensors).

    Without `base` every non-LoRA tensor stays in the returned base state dict and the adapter holds the pairs only.
    With `base` (the plain state dict of the resident model) the checkpoint is read AGAINST it: a non-LoRA tensor equal
    to the base's is dropped, one that differs becomes a replacement tensor of the adapter -- or raises if it is not
    replaceable -- and a `base_layer` that differs from the base raises (the adapter was trained on another model).
    The returned base state dict is then `base` itself."""
    plain = _strip(state_dict)
    ckpt_base, tensors = {}, {}
    for k, v in plain.items():
        m = re.match(r"^(.*)\.lora_([AB])\.default\.weight$", k)
        if m is not None:
            tensors[f"{m.group(1)}.lora_{m.group(2)}.weight"] = v
        elif ".base_layer." in k:
            ckpt_base[k.replace(".base_layer.", ".")] = v
        else:
            ckpt_base.setdefault(k, v)
    if base is None:
        return ckpt_base, tensors
    lora_weights = {k[: -len(".lora_A.weight")] + ".weight" for k in tensors if k.endswith(".lora_A.weight")}
    for k, v in ckpt_base.items():
        if k not in base:
            raise ValueError(f"{k!r} of the checkpoint is not a tensor of the base model")
        same = tuple(v.shape) == tuple(base[k].shape) and torch.equal(v.to(torch.float32), base[k].to(torch.float32))
        if same:
            continue
        if k in lora_weights or not is_replaceable(k):
            what = "base_layer" if k in lora_weights else "tensor"
            raise ValueError(f"{what} {k!r} of the checkpoint differs from the base model and is not replaceable "
                             f"(only {FULL_PREFIX}* is): the adapter belongs to another base")
        tensors[k] = v
    return base, tensors


def lowrank_term(a: torch.Tensor, b: torch.Tensor, rule: str = "contract") -> torch.Tensor:
    """B A in fp32.  "matmul": torch's `b @ a` (the reference).  "contract": the engine's rule -- per element
    acc = acc + B[o][r] * A[r][i] for ascending r, the product rounded before the add (no fused multiply-add)."""
    a, b = a.to(torch.float32), b.to(torch.float32)
    if rule == "matmul":
        return b @ a
    if rule != "contract":
        raise ValueError(f"unknown merge rule {rule!r}")
    acc = torch.zeros(b.shape[0], a.shape[1], dtype=torch.float32)
    for r in range(a.shape[0]):
        acc = acc + b[:, r:r + 1] * a[r:r + 1, :]
    return acc


def merge_adapter(base: dict, tensors: dict, *, lora_alpha=32, lora_r=16, alpha_pattern=None, rank_pattern=None,
                  rule: str = "contract") -> dict:
    """The plain state dict of `base` with an adapter merged on the host: W + (B A) * scale for every pair,
    replacement tensors swapped in.  rule="contract" gives exactly the weights the engine holds after set_adapter."""
    pairs, full = split_adapter_tensors(tensors)
    out = dict(base)
    for mod, (a, b) in pairs.items():
        w = base[mod + ".weight"]
        if tuple(w.shape) != (b.shape[0], a.shape[1]):
            raise ValueError(f"{mod}: lora_A {tuple(a.shape)} / lora_B {tuple(b.shape)} do not fit the weight {tuple(w.shape)}")
        scale = pair_scale(mod, lora_alpha, lora_r, alpha_pattern, rank_pattern)
        out[mod + ".weight"] = (w.to(torch.float32) + lowrank_term(a, b, rule) * scale).to(w.dtype)
    for k, v in full.items():
        if tuple(v.shape) != tuple(base[k].shape):
            raise ValueError(f"{k}: shape {tuple(v.shape)} != {tuple(base[k].shape)}")
        out[k] = v
    return out
