"""Backbones with the reference's protocol -- `forward(x, cond, text, time, mask, drop_audio_cond, drop_text,
cfg_infer, cache)`, `.dim`, `.clear_cache()` (model/backbones/dit.py:146-329, unett.py:107-280) -- whose arithmetic
runs entirely in libf5hip (HIP kernels).  Parameters keep the reference's state-dict names so checkpoints load as is.
"""
from __future__ import annotations

import torch
from torch import nn

from . import adapters as A
from . import weights as W
from .config import normalize_arch
from .engine import Engine


def valid_length_bucket(granule: int) -> bool:
    return granule == 0 or (8 <= granule <= 1024 and granule % 8 == 0)


def bucket_ceiling(n: int, granule: int) -> int:
    """The length a sample() call of n frames is planned at under a length bucket of `granule` frames (0: n itself)."""
    return n if not granule else -(-n // granule) * granule


class _HipBackbone(nn.Module):
    backbone_name = "DiT"

    def __init__(self, *, mel_dim=100, text_num_embeds=256, precision="parity", device=None, max_pos=8192, **arch):
        super().__init__()
        self.length_bucket = 0              # granule of the length-bucketed sample() graphs; 0: off (set_length_buckets)
        self.isolated_rows = False          # sample_items() / sample_span() on packed rows, each row as if alone (set_isolated_rows)
        self.graph_capacity = 0             # graphs the engine's cache holds; 0: the engine's default of 16 (set_graph_capacity)
        # "parity" (the default): the fastest operand precision measured inside the 1e-3 mel bar of the fp32 CPU path for THIS backbone
        # (DESIGN.md section 3): DiT "f16p" (f16 blocks, split-f16 input / output layers); the E2-TTS UNetT has no AdaLN gates and
        # every one of its GEMM classes costs ~1e-3 in plain f16, so it gets "f16x3" (split-f16 GEMM products, f16 attention products)
        # the MMDiT: "f16x3" too -- against the reference's vectors at its fixtures' weight scale f16p reaches 1.5e-3
        if precision == "parity":
            precision = "f16p" if self.backbone_name == "DiT" else "f16x3"
        # "f8" (never the default): "f16p" with e4m3 operands in the four GEMMs of every DiT block (include/f5_hip.h F5_PREC_F8)
        if precision in ("f8", "fp8"):
            precision = "f8"
            if self.backbone_name != "DiT":
                raise NotImplementedError(f"precision 'f8' is built for the DiT backbone only, not the {self.backbone_name}")
        arch.pop("dropout", None)
        arch.pop("attn_backend", None)          # one attention implementation: the gfx950 flash kernel
        arch.pop("checkpoint_activations", None)
        self.arch = normalize_arch(arch, mel_dim)
        self.dim = self.arch["dim"]
        self.depth = self.arch["depth"]
        self.mel_dim = mel_dim
        self.text_num_embeds = text_num_embeds
        self.precision = precision
        self.max_pos = max_pos
        self._device = torch.device(device) if device is not None else None
        self._sd: dict[str, torch.Tensor] = {}
        self._engine: Engine | None = None
        self._adapters: dict[str, tuple[dict, dict]] = {}   # name -> ({module: (A, B, scale)}, {name: replacement tensor}), host fp32
        self._adapter_handles: dict[str, object] = {}       # name -> f5_adapter handle of the current engine
        self.active_adapter: str | None = None
        self._anchor = nn.Parameter(torch.zeros(1), requires_grad=False)  # lets `.to(device)` / `.device` work

    # ---- shapes / state dict -------------------------------------------------------------------------
    def param_shapes(self):
        fn = {"DiT": W.dit_param_shapes, "UNetT": W.unett_param_shapes, "MMDiT": W.mmdit_param_shapes}[self.backbone_name]
        return fn(self.arch, self.text_num_embeds, self.mel_dim)

    def init_synthetic(self, seed: int = 0):
        """Deterministic random weights (see weights.synthetic_state_dict); used by tests and bench."""
        self.load_state_dict(W.synthetic_state_dict(self.param_shapes(), seed=seed))
        return self

    def state_dict(self, *a, **k):  # noqa: D401 - reference names, fp32 host copies
        return dict(self._sd)

    def load_state_dict(self, sd, strict=True, assign=False):
        sd = W.strip_prefixes(sd)
        shapes = self.param_shapes()
        missing = [k for k in shapes if k not in sd]
        unexpected = [k for k in sd if k not in shapes]
        if strict and (missing or unexpected):
            raise RuntimeError(f"state dict mismatch: missing {missing[:4]}..., unexpected {unexpected[:4]}...")
        for k, shp in shapes.items():
            if k in sd and tuple(sd[k].shape) != tuple(shp):
                raise RuntimeError(f"{k}: shape {tuple(sd[k].shape)} != {tuple(shp)}")
        self._sd = {k: sd[k].detach().to("cpu", torch.float32) for k in shapes if k in sd}
        self._drop_engine()  # re-upload lazily on the current device
        return nn.modules.module._IncompatibleKeys(missing, unexpected)

    # ---- engine ----------------------------------------------------------------------------------------
    @property
    def device(self):
        return self._anchor.device

    def engine(self) -> Engine:
        dev = self._anchor.device
        if dev.type != "cuda":
            raise RuntimeError("the HIP backbone only runs on a GPU: call .to('cuda') first (there is no CPU path)")
        if self._engine is None or self._engine.device != dev:
            if not self._sd:
                raise RuntimeError("no weights loaded: call load_state_dict() or init_synthetic()")
            self._drop_engine()
            e = Engine(self.arch, self.text_num_embeds, self.mel_dim, backbone=self.backbone_name,
                       precision=self.precision, device=dev, max_pos=self.max_pos, adapters=bool(self._adapters))
            e.load_state_dict(self._sd)
            if self.length_bucket:
                e.set_length_buckets(self.length_bucket)
            if self.isolated_rows:
                e.set_isolated_rows(True)
            if self.graph_capacity:
                e.set_graph_capacity(self.graph_capacity)
            self._engine = e
            for name, (pairs, full) in self._adapters.items():
                self._adapter_handles[name] = e.new_adapter(pairs, full)
            if self.active_adapter is not None:
                e.set_adapter(self._adapter_handles[self.active_adapter])
        return self._engine

    def _drop_engine(self):
        """Forgets the engine (and the adapter handles that belong to it); the next engine() builds a new one."""
        self._adapter_handles = {}   # (the Engine frees them with itself)
        self._engine = None

    # ---- length-bucketed sample() graphs ------------------------------------------------------------------------
    def set_length_buckets(self, granule: int):
        """Plans eligible sample() calls at their length rounded up to `granule` frames (a multiple of 8 in [8, 1024]; 0: off),
        so that one captured HIP graph serves every length of a bucket; results do not change.  Survives engine rebuilds."""
        if self.backbone_name != "DiT":
            raise NotImplementedError("length buckets are built for the DiT backbone only")
        granule = int(granule)
        if not valid_length_bucket(granule):
            raise ValueError(f"length bucket {granule}: expected 0 (off) or a multiple of 8 in [8, 1024]")
        self.length_bucket = granule
        if self._engine is not None:
            self._engine.set_length_buckets(granule)
            if self.graph_capacity:                      # (the engine's setter puts the cache back to 16 graphs)
                self._engine.set_graph_capacity(self.graph_capacity)

    # ---- isolated rows -------------------------------------------------------------------------------------------
    def set_isolated_rows(self, on: bool):
        """sample_items() and sample_span() run every row as if it were alone in the batch: on packed rows, with the row's own length
        masking attention keys and conv-pos whatever `attn_mask_enabled` says, and in the engine's length buckets when those are on.
        Inside its own frames a row then equals the same item at B = 1, bit for bit, in any batch.  A call that cannot keep that
        (F5_SPLIT_CFG=1, text_embedding_average_upsampling, a length past the position tables) raises instead of running
        rectangular.  sample() is untouched.  Off by default; survives engine rebuilds."""
        if on and self.backbone_name != "DiT":
            raise NotImplementedError("isolated rows run on packed rows, which are built for the DiT backbone only")
        self.isolated_rows = bool(on)
        if self._engine is not None:
            self._engine.set_isolated_rows(self.isolated_rows)

    def set_graph_capacity(self, n: int):
        """The engine's graph cache holds n graphs (16 to 64), for callers whose batches vary in size as well as in length bucket.
        Survives engine rebuilds and set_length_buckets."""
        n = int(n)
        if not 16 <= n <= 64:
            raise ValueError(f"graph capacity {n}: expected 16 to 64 graphs")
        self.graph_capacity = n
        if self._engine is not None:
            self._engine.set_graph_capacity(n)

    def prepare_sample(self, batch: int, n_min: int, n_max: int, nt_max: int, steps: int, cfg_strength: float, *,
                       method: str = "euler", want_traj: bool = True):
        """Captures the graphs of every length bucket that durations n_min .. n_max touch before the first request
        (CFM.sample's arguments: steps after any duplicate_test shortening, texts of at most nt_max tokens)."""
        if self.backbone_name != "DiT":
            raise NotImplementedError("length buckets are built for the DiT backbone only")
        self.engine().prepare_sample(batch, n_min, n_max, nt_max, steps, cfg_strength, method=method, want_traj=want_traj)

    def graph_stats(self, reset: bool = False) -> dict:
        return self.engine().graph_stats(reset)

    # ---- resident LoRA adapters (the interface PEFT users know: add / set / delete) ---------------------------
    @property
    def adapters(self) -> list[str]:
        return list(self._adapters)

    def add_adapter(self, name: str, tensors: dict, *, lora_alpha=32, lora_r=16, alpha_pattern=None, rank_pattern=None):
        """Registers a LoRA fine-tune of the loaded weights under `name` without activating it.  `tensors`:
        `<module>.lora_A.weight` [r, in] / `<module>.lora_B.weight` [out, r] for to_q / to_k / to_v / to_out.0 of any DiT
        block and input_embed.proj (any rank 1 .. 128 per pair), and full replacements of `text_embed.*` tensors under
        their own names.  A pair's scale is alpha / r with PEFT's alpha_pattern / rank_pattern overrides (the reference's
        recipe, train/train_lora.py: 32 / 16, and {"input_embed.proj": 128} / {"input_embed.proj": 64}).
        The first adapter added after the engine was built rebuilds the engine once (it has to keep fp32 masters);
        later adds upload to the resident engine, and set_adapter() never rebuilds."""
        if self.backbone_name != "DiT":
            raise NotImplementedError("resident adapters are built for the DiT backbone only")
        if self.precision == "f8":
            raise NotImplementedError("resident adapters are not built for precision 'f8': a switch merges into packed 16-bit "
                                      "operands, and re-quantising e4m3 weights on a switch is a later step")
        if name in self._adapters:
            raise ValueError(f"adapter {name!r} exists: delete_adapter() it first")
        pairs, full = A.split_adapter_tensors(W.strip_prefixes(tensors))
        shapes = self.param_shapes()
        host_pairs = {}
        for mod, (a, b) in pairs.items():
            shp = shapes.get(mod + ".weight")
            if shp is None or tuple(shp) != (b.shape[0], a.shape[1]):
                raise ValueError(f"{mod}: lora_A {tuple(a.shape)} / lora_B {tuple(b.shape)} do not fit the weight {shp}")
            host_pairs[mod] = (a.detach().to("cpu", torch.float32), b.detach().to("cpu", torch.float32),
                               A.pair_scale(mod, lora_alpha, lora_r, alpha_pattern, rank_pattern))
        for k, v in full.items():
            if k not in shapes or tuple(shapes[k]) != tuple(v.shape):
                raise ValueError(f"{k}: shape {tuple(v.shape)} != {shapes.get(k)}")
        host_full = {k: v.detach().to("cpu", torch.float32) for k, v in full.items()}
        self._adapters[name] = (host_pairs, host_full)
        if self._engine is not None:
            if not self._engine.adapters:
                self._drop_engine()          # built without F5_OPT_ADAPTERS: rebuilt, once, by the next engine()
            else:
                self._adapter_handles[name] = self._engine.new_adapter(host_pairs, host_full)

    def set_adapter(self, name: str | None):
        """Switches the resident model to adapter `name` (None: the base weights): one kernel launch that rewrites the
        packed weights in place; captured graphs, the arena and every other weight stay."""
        if name is not None and name not in self._adapters:
            raise KeyError(f"no adapter {name!r} (have {self.adapters})")
        self.active_adapter = name
        if self._engine is not None and self._engine.adapters:
            self._engine.set_adapter(None if name is None else self._adapter_handles[name])

    def delete_adapter(self, name: str):
        if name not in self._adapters:
            raise KeyError(f"no adapter {name!r} (have {self.adapters})")
        if name == self.active_adapter:
            raise RuntimeError(f"adapter {name!r} is active: set_adapter() another one (or None) first")
        del self._adapters[name]
        h = self._adapter_handles.pop(name, None)
        if h is not None and self._engine is not None:
            self._engine.free_adapter(h)

    def clear_cache(self):
        """The reference clears its per-sample() text cache here (dit.py:275-276); the engine keeps no state
        between calls, so there is nothing to clear."""
        return None

    def forward(self, x, cond, text, time, mask=None, drop_audio_cond=False, drop_text=False, cfg_infer=False,
                cache=False):
        lens = None
        if mask is not None:
            lens = mask.sum(dim=1).tolist()
        t = time.reshape(-1).tolist() if isinstance(time, torch.Tensor) else [float(time)]
        out = self.engine().forward(x, cond, text, t, lens=lens, cfg_infer=cfg_infer, drop_audio_cond=drop_audio_cond,
                                    drop_text=drop_text)
        return out.to(x.dtype)


class DiT(_HipBackbone):
    backbone_name = "DiT"


class UNetT(_HipBackbone):
    backbone_name = "UNetT"

    def __init__(self, *, skip_connect_type="concat", **kw):
        if skip_connect_type != "concat":
            raise NotImplementedError("only skip_connect_type='concat' (the E2TTS configs) is built")
        super().__init__(**kw)


class MMDiT(_HipBackbone):
    """The reference's MMDiT (backbones/mmdit.py:85-213): a text stream and an audio stream with their own weights, joined in one
    attention per block.  Constructor keywords are the reference's; `dropout` is accepted and ignored.  A batch runs rectangular
    (the input conv is unmasked), so the packed-row features -- length buckets, isolated rows, per-item and sliced solves -- and the
    resident adapters stay with the DiT."""
    backbone_name = "MMDiT"

    def __init__(self, *, dim, depth=8, heads=8, dim_head=64, dropout=0.1, ff_mult=4, mel_dim=100, text_num_embeds=256,
                 text_mask_padding=True, qk_norm=None, precision="parity", device=None, max_pos=8192):
        if qk_norm not in (None, "rms_norm"):
            raise ValueError(f"Unimplemented qk_norm: {qk_norm}")                       # modules.py:404
        if dim_head != 64:
            raise ValueError(f"dim_head must be 64 (got {dim_head}): the attention kernels are built for it")
        # (the text stream has the model's width; there is no ConvNeXt, every head is rotated, a mask that is given is applied)
        super().__init__(mel_dim=mel_dim, text_num_embeds=text_num_embeds, precision=precision, device=device, max_pos=max_pos,
                         dim=dim, depth=depth, heads=heads, dim_head=dim_head, ff_mult=ff_mult, text_dim=dim, conv_layers=0,
                         text_mask_padding=text_mask_padding, qk_norm=qk_norm, pe_attn_head=None, attn_mask_enabled=True)
