"""CPU: the host side of the resident LoRA adapters -- splitting a PEFT checkpoint into (base, adapter), the host merges, the
pair scales, the Python registry on the backbone -- and the C ABI's new symbols (declared, exported, bound, null handles
rejected).  The device side is tests/test_adapters_gpu.py."""
import ctypes as C
import os
import re

import pytest
import torch

import adapter_util as U
from conftest import ROOT, load_golden, synthetic_weights

import f5_tts_amd as P
from f5_tts_amd import _lib, adapters as A
from f5_tts_amd import infer as I

NEW_SYMBOLS = ["f5_adapter_create", "f5_adapter_destroy", "f5_adapter_put_lora", "f5_adapter_put_tensor", "f5_set_adapter"]


def fixture(name="sample_b1_nfe16"):
    meta, a = load_golden(name)
    return meta, a, synthetic_weights(meta)


def test_split_and_matmul_merge_equals_convert_peft_state_dict_to_plain():
    meta, _, sd = fixture()
    t = U.synth_adapter(sd, meta["arch"]["depth"], seed=1)
    ck = U.peft_checkpoint(sd, t)
    # the checkpoint as load_checkpoint sees it: `ema_model.` off, then the reference's merge (alpha / r = 2 everywhere)
    plain = I.convert_peft_state_dict_to_plain({k.replace("ema_model.", ""): v for k, v in ck.items()})
    plain = P.weights.strip_prefixes(plain)
    # read without a base: every non-LoRA tensor is "base", the adapter is the pairs
    base0, t0 = A.split_peft_state_dict(ck)
    assert sorted(base0) == sorted(sd) and all(".lora_" in k for k in t0)
    merged0 = A.merge_adapter(base0, t0, rule="matmul", **U.RECIPE)
    assert sorted(merged0) == sorted(plain) and all(torch.equal(merged0[k], plain[k]) for k in plain)
    # read against the resident base: equal tensors dropped, the trained text encoder kept as replacement tensors
    base1, t1 = A.split_peft_state_dict(ck, base=sd)
    assert base1 is sd
    assert sorted(t1) == sorted(t) and all(torch.equal(t1[k], t[k]) for k in t)
    merged1 = A.merge_adapter(sd, t1, rule="matmul", **U.RECIPE)
    assert all(torch.equal(merged1[k], plain[k]) for k in plain)
    changed = [k for k in sd if not torch.equal(sd[k], merged1[k])]
    assert len(changed) == 4 * meta["arch"]["depth"] + 1 + sum(k.startswith("text_embed.") for k in sd)


def test_split_drops_equal_tensors_and_rejects_a_foreign_base():
    meta, _, sd = fixture()
    t = U.synth_adapter(sd, meta["arch"]["depth"], seed=2, blocks=[1], in_rank=0, text=False)
    ck = U.peft_checkpoint(sd, t)
    _, t1 = A.split_peft_state_dict(ck, base=sd)
    assert sorted(t1) == sorted(t)                                   # no full tensor: the text encoder equals the base's
    bad = dict(ck)
    k = "ema_model.base_model.model.transformer.transformer_blocks.1.attn.to_q.base_layer.weight"
    bad[k] = bad[k] + 1e-3
    with pytest.raises(ValueError, match="transformer_blocks.1.attn.to_q.weight"):
        A.split_peft_state_dict(bad, base=sd)
    bad = dict(ck)
    k = "ema_model.base_model.model.transformer.proj_out.bias"       # differs, and is not replaceable
    bad[k] = bad[k] + 1e-3
    with pytest.raises(ValueError, match="proj_out.bias"):
        A.split_peft_state_dict(bad, base=sd)


def test_contract_merge_is_a_rounded_product_then_add_in_ascending_rank():
    g = torch.Generator().manual_seed(0)
    a, b = torch.randn(24, 40, generator=g), torch.randn(12, 24, generator=g)
    got = A.lowrank_term(a, b, "contract")
    want = torch.zeros(12, 40)
    for o in range(12):
        for i in range(40):
            acc = torch.zeros((), dtype=torch.float32)
            for r in range(24):
                acc = acc + b[o, r] * a[r, i]
            want[o, i] = acc
    assert torch.equal(got, want)
    assert (got - b @ a).abs().max() < 1e-5 and (got.double() - b.double() @ a.double()).abs().max() < 1e-5


def test_pair_scale_follows_the_peft_patterns():
    r = U.RECIPE
    assert A.pair_scale("transformer_blocks.3.attn.to_q", **r) == 2.0
    assert A.pair_scale("input_embed.proj", **r) == 2.0
    assert A.pair_scale("input_embed.proj", 32, 16, {"input_embed.proj": 96}, {"input_embed.proj": 64}) == 1.5
    assert A.pair_scale("transformer_blocks.0.attn.to_out.0", 12, 16) == 0.75
    assert A.pair_scale("transformer_blocks.0.attn.to_out.0", 32, 16, {r"to_out\.0": 8}, None) == 0.5


def test_backbone_registry_and_name_checks_need_no_gpu():
    meta, _, sd = fixture()
    tr = P.DiT(**meta["arch"], text_num_embeds=meta["nvocab"], mel_dim=100, precision="f32")
    tr.load_state_dict(sd)
    assert tr.adapters == [] and tr.active_adapter is None
    t = U.synth_adapter(sd, meta["arch"]["depth"], seed=1)
    tr.add_adapter("a", t, **U.RECIPE)
    tr.add_adapter("b", {k: v for k, v in t.items() if ".lora_" in k and "blocks.0." in k}, lora_alpha=12)
    assert tr.adapters == ["a", "b"]
    tr.set_adapter("a")
    assert tr.active_adapter == "a"
    with pytest.raises(RuntimeError):
        tr.delete_adapter("a")
    with pytest.raises(KeyError):
        tr.set_adapter("nope")
    with pytest.raises(ValueError):
        tr.add_adapter("a", t)
    tr.set_adapter(None)
    tr.delete_adapter("a")
    assert tr.adapters == ["b"]
    for bad, pat in [({"proj_out.weight": sd["proj_out.weight"]}, "proj_out.weight"),
                     ({"transformer_blocks.0.ff.ff.2.lora_A.weight": torch.zeros(4, 512),
                       "transformer_blocks.0.ff.ff.2.lora_B.weight": torch.zeros(256, 4)}, "ff.ff.2"),
                     ({"input_embed.proj.lora_A.weight": torch.zeros(4, 264)}, "input_embed.proj"),
                     ({"input_embed.proj.lora_A.weight": torch.zeros(4, 260), "input_embed.proj.lora_B.weight": torch.zeros(256, 4)},
                      "input_embed.proj"),
                     ({"input_embed.proj.lora_A.weight": torch.zeros(129, 264), "input_embed.proj.lora_B.weight": torch.zeros(256, 129)},
                      "input_embed.proj"),
                     ({"text_embed.text_embed.weight": torch.zeros(3, 64)}, "text_embed.text_embed.weight")]:
        with pytest.raises(ValueError, match=re.escape(pat)):
            tr.add_adapter("x", bad)
    un = P.UNetT(dim=256, depth=2, heads=4, ff_mult=2, text_dim=64, conv_layers=0, text_num_embeds=40, mel_dim=100)
    with pytest.raises(NotImplementedError):
        un.add_adapter("a", {})


def test_load_adapter_reads_a_peft_checkpoint_against_the_loaded_base(tmp_path):
    meta, _, sd = fixture()
    t = U.synth_adapter(sd, meta["arch"]["depth"], seed=3)
    path = str(tmp_path / "ft.pt")
    torch.save({"ema_model_state_dict": dict(U.peft_checkpoint(sd, t), **{"initted": torch.tensor(True), "step": torch.tensor(7)})}, path)
    tr = P.DiT(**meta["arch"], text_num_embeds=meta["nvocab"], mel_dim=100, precision="f32")
    tr.load_state_dict(sd)
    I.load_adapter(tr, path, "ft", **{k: v for k, v in U.RECIPE.items()})
    pairs, full = tr._adapters["ft"]
    assert len(pairs) == 4 * meta["arch"]["depth"] + 1 and all(s == 2.0 for _, _, s in pairs.values())
    assert sorted(full) == sorted(k for k in sd if k.startswith("text_embed."))
    assert torch.equal(pairs["input_embed.proj"][0], t["input_embed.proj.lora_A.weight"])


def test_new_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "f5_hip.h")).read()
    assert re.search(r"#define\s+F5_OPT_ADAPTERS\s+8\b", hdr) and _lib.F5_OPT_ADAPTERS == 8
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\bint\s+{name}\s*\(", hdr), f"{name} is not declared in include/f5_hip.h"
        assert hasattr(lib, name) and name in _lib.SIGNATURES


def test_null_handles_are_rejected_without_a_gpu():
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.f5_set_adapter(None, None, None) == -1 and b"null engine" in lib.f5_last_error()
    assert lib.f5_adapter_create(None, C.byref(h)) == -1
    assert lib.f5_adapter_put_lora(None, b"input_embed.proj.weight", None, None, 0, None, None, 0, 1.0, None) == -1
    assert b"null adapter" in lib.f5_last_error()
    assert lib.f5_adapter_put_tensor(None, b"text_embed.text_embed.weight", None, None, 0, None) == -1
    assert lib.f5_adapter_destroy(None) == 0            # like free(NULL)
    # the option bit is a DiT option: f5_create rejects it for UNetT
    cfg = _lib.f5_config()
    cfg.backbone, cfg.dim, cfg.depth, cfg.heads, cfg.dim_head, cfg.ff_dim = _lib.F5_BACKBONE_UNETT, 256, 2, 4, 64, 512
    cfg.text_dim, cfg.mel_dim, cfg.options = 64, 100, _lib.F5_OPT_ADAPTERS
    assert lib.f5_create(C.byref(cfg), C.byref(h)) == -1 and b"DiT" in lib.f5_last_error()
