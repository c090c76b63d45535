"""Seeded synthetic LoRA adapters for tests/test_adapters*.py (plain adapter-tensor names, korean-f5-tts_amd/adapters.py)
and the PEFT-style checkpoint train/train_lora.py would have written for them."""
import torch

ATTN = ("to_q", "to_k", "to_v", "to_out.0")
RECIPE = dict(lora_alpha=32, lora_r=16, alpha_pattern={"input_embed.proj": 128}, rank_pattern={"input_embed.proj": 64})
# Magnitude of the synthetic fine-tune: the standard deviation of the merged update s * B A of every adapted weight (the base
# weights have 0.02) and of the noise added to the replaced text-encoder tensors.  Chosen on the CPU (test_adapters.py checks
# it there) so that the oracle's trajectory with the adapter differs from the one without by more than 10 x the widest
# parity gate (bf16: 3e-2) on both fixtures.
DELTA_STD = 0.02
TEXT_STD = 0.1


def pair(gen, out, inn, rank, scale, delta_std=DELTA_STD):
    """A [rank, in], B [out, rank] with std(scale * B A) = delta_std."""
    s = (delta_std / (abs(scale) * rank ** 0.5)) ** 0.5
    return torch.randn(rank, inn, generator=gen) * s, torch.randn(out, rank, generator=gen) * s


def synth_adapter(sd, depth, seed, *, ranks=16, in_rank=64, blocks=None, mods=ATTN, scale=2.0, text=True, delta_std=DELTA_STD,
                  text_std=TEXT_STD):
    """Adapter tensors on `mods` of `blocks` (None: all) with per-module `ranks` (an int, or {module suffix: rank}),
    rank `in_rank` on input_embed.proj (0: none), and every text_embed.* tensor replaced (`text`).  `scale` is the one the
    caller will apply (only used to size the pair)."""
    g = torch.Generator().manual_seed(seed)
    t = {}
    for i in (range(depth) if blocks is None else blocks):
        for m in mods:
            w = sd[f"transformer_blocks.{i}.attn.{m}.weight"]
            r = ranks[m] if isinstance(ranks, dict) else ranks
            a, b = pair(g, w.shape[0], w.shape[1], r, scale, delta_std)
            t[f"transformer_blocks.{i}.attn.{m}.lora_A.weight"] = a
            t[f"transformer_blocks.{i}.attn.{m}.lora_B.weight"] = b
    if in_rank:
        w = sd["input_embed.proj.weight"]
        a, b = pair(g, w.shape[0], w.shape[1], in_rank, scale, delta_std)
        t["input_embed.proj.lora_A.weight"], t["input_embed.proj.lora_B.weight"] = a, b
    if text:
        for k, v in sd.items():
            if k.startswith("text_embed."):
                t[k] = v + torch.randn(v.shape, generator=g) * text_std * (1.0 if k.endswith("text_embed.weight") else 0.2)
    return t


def peft_checkpoint(sd, tensors, prefix="ema_model.base_model.model.transformer."):
    """The state dict a PEFT-wrapped model saves for base `sd` + adapter `tensors`: `.base_layer.` on the wrapped linears,
    `.lora_A/B.default.weight`, everything else (trained text encoder included) under its own name."""
    wrapped = {k[: -len(".lora_A.weight")] for k in tensors if k.endswith(".lora_A.weight")}
    out = {}
    for k, v in sd.items():
        mod, _, leaf = k.rpartition(".")
        if mod in wrapped:
            out[f"{prefix}{mod}.base_layer.{leaf}"] = v
        else:
            out[prefix + k] = tensors.get(k, v)
    for k, v in tensors.items():
        if ".lora_" in k:
            mod, ab, _ = k.rsplit(".", 2)
            out[f"{prefix}{mod}.{ab}.default.weight"] = v
    return out
