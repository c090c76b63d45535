"""Thin Python owner of one libf5hip engine handle: uploads weights, passes raw device pointers + the current HIP stream.

PyTorch is used only for device memory (torch.Tensor.data_ptr), the current stream and host-side constant tables.
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib
from ._lib import _dev_f32, _ptr, _stream_ptr  # noqa: F401  (`from .engine import _ptr` keeps working)
from .config import normalize_arch


def _h2d_async(t: torch.Tensor, device, dtype) -> torch.Tensor:
    """Host tensor -> device without blocking the host: a pageable `.to(device)` waits for everything already queued on
    the stream (the previous utterance's whole ODE solve), which serialises the host's per-call work with the GPU.
    Staged through torch's caching pinned allocator (it keeps the block alive until the copy has executed)."""
    t = t.detach().to(dtype).contiguous()
    if t.device.type != "cpu":
        return t.to(device)
    return t.pin_memory().to(device, non_blocking=True)


def aux_tables(dim_head: int, max_pos: int, text_dim: int, text_pos_rows: int) -> dict[str, torch.Tensor]:
    """Host-computed constant tables, evaluated with the same torch fp32 ops the reference uses:
    rotary angles (x_transformers RotaryEmbedding as called at dit.py:184,311; restated in-repo at
    runtime/triton_trtllm/model_repo_f5_tts/f5_tts/1/f5_tts_trtllm.py:230-237), the sinusoidal time frequencies
    (modules.py:159-161) and the text position table precompute_freqs_cis (modules.py:202-213)."""
    inv_freq = 1.0 / (10000.0 ** (torch.arange(0, dim_head, 2).float() / dim_head))
    ang = torch.einsum("i,j->ij", torch.arange(max_pos).type_as(inv_freq), inv_freq)  # [max_pos, dh/2]
    half = 128
    tf = torch.exp(torch.arange(half).float() * -(math.log(10000) / (half - 1)))
    out = {"aux.rope_cos": ang.cos(), "aux.rope_sin": ang.sin(), "aux.time_freqs": tf}
    if text_pos_rows > 0:
        freqs = 1.0 / (10000.0 ** (torch.arange(0, text_dim, 2)[: text_dim // 2].float() / text_dim))
        a = torch.outer(torch.arange(text_pos_rows), freqs).float()
        out["aux.text_pos"] = torch.cat([a.cos(), a.sin()], dim=-1)
    return out


class Engine:
    """One f5_engine handle bound to one device (one process per GPU; handles are not shared across streams)."""

    def __init__(self, arch: dict, text_num_embeds: int, mel_dim: int = 100, *, backbone: str = "DiT",
                 precision: str = "f16p", device="cuda", max_pos: int = 8192, adapters: bool = False):
        self.lib = _lib.load()  # raises if the HIP library is not built
        if not torch.cuda.is_available():
            raise _lib.F5Error("no GPU visible: the F5-TTS engine has no CPU path")
        self.device = torch.device(device if device != "cuda" else f"cuda:{torch.cuda.current_device()}")
        a = normalize_arch(arch, mel_dim)
        self.arch = a
        self.backbone = backbone
        self.precision = precision
        self.mel_dim = mel_dim
        self.text_num_embeds = text_num_embeds
        self.max_pos = max_pos
        cfg = _lib.f5_config()
        cfg.backbone = _lib.BACKBONES[backbone]
        cfg.precision = _lib.PRECISIONS[precision]
        cfg.dim, cfg.depth, cfg.heads, cfg.dim_head = a["dim"], a["depth"], a["heads"], a["dim_head"]
        cfg.ff_dim = int(a["dim"] * a["ff_mult"])
        cfg.text_dim, cfg.conv_layers = a["text_dim"], a["conv_layers"]
        cfg.pe_attn_head = -1 if a["pe_attn_head"] is None else int(a["pe_attn_head"])
        cfg.text_mask_padding = int(bool(a["text_mask_padding"]))
        cfg.attn_mask_enabled = int(bool(a["attn_mask_enabled"]))
        cfg.text_num_embeds, cfg.mel_dim, cfg.max_pos = text_num_embeds, mel_dim, max_pos
        if a.get("qk_norm") not in (None, "rms_norm"):
            raise ValueError(f"Unimplemented qk_norm: {a['qk_norm']}")                       # modules.py:404
        if a.get("qk_norm") and backbone == "UNetT":
            raise _lib.F5Error("qk_norm / long_skip_connection / text_embedding_average_upsampling are DiT options")
        if (a.get("long_skip_connection") or a.get("text_embedding_average_upsampling")) and backbone != "DiT":
            raise _lib.F5Error("qk_norm / long_skip_connection / text_embedding_average_upsampling are DiT options")
        if a.get("text_embedding_average_upsampling") and not a["text_mask_padding"]:
            raise AssertionError("text_embedding_average_upsampling requires text_mask_padding to be True")   # dit.py:41-42
        cfg.options = ((_lib.F5_OPT_QK_RMSNORM if a.get("qk_norm") else 0) | (_lib.F5_OPT_LONG_SKIP if a.get("long_skip_connection") else 0) |
                       (_lib.F5_OPT_TEXT_AVG_UPSAMPLE if a.get("text_embedding_average_upsampling") else 0))
        # resident LoRA adapters (F5_OPT_ADAPTERS): the engine keeps the fp32 masters of the adaptable tensors
        if adapters and backbone != "DiT":
            raise _lib.F5Error("resident adapters are built for the DiT backbone only")
        self.adapters = bool(adapters)
        cfg.options |= _lib.F5_OPT_ADAPTERS if adapters else 0
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.f5_create(C.byref(cfg), C.byref(self._h)), "f5_create")
        self.ready = False
        self._adapter_handles: list = []   # live f5_adapter handles of this engine (freed with it)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                self.lib.f5_destroy(h)
                for a in getattr(self, "_adapter_handles", []):   # (after the engine: none of them is "active" any more)
                    self.lib.f5_adapter_destroy(a)
            except Exception:
                pass
            self._h = None

    # ------------------------------------------------------------------ weights
    def load_state_dict(self, sd: dict[str, torch.Tensor]):
        a = self.arch
        text_rows = 0
        if a["conv_layers"] > 0:
            text_rows = 8192 if self.backbone == "DiT" else 4096  # dit.py:46 / unett.py:46
        if self.backbone == "MMDiT":
            text_rows = 1024                                      # mmdit.py:37-38 (the reference's buffer is non-persistent: built here)
        tables = aux_tables(a["dim_head"], self.max_pos, a["text_dim"], text_rows)
        with torch.cuda.device(self.device):
            st = _stream_ptr(self.device)
            for name, t in list(sd.items()) + list(tables.items()):
                d = _dev_f32(t, self.device)
                _lib.check(self.lib.f5_load_weight(self._h, name.encode(), _ptr(d), _lib.shape_array(d.shape), d.dim(),
                                                   st), f"f5_load_weight({name})")
            _lib.check(self.lib.f5_finalize(self._h, st), "f5_finalize")
        self.ready = True

    def reserve(self, max_batch: int, max_frames: int, max_steps: int = 32):
        with torch.cuda.device(self.device):
            _lib.check(self.lib.f5_reserve(self._h, max_batch, max_frames, max_steps), "f5_reserve")

    # ------------------------------------------------------------------ length buckets
    def set_length_buckets(self, granule: int):
        """0: off.  Else a multiple of 8 in [8, 1024]: eligible sample() calls are planned at N rounded up to it, so that one
        captured graph serves every length of a bucket (include/f5_hip.h).  Clears the graph cache."""
        _lib.check(self.lib.f5_set_length_buckets(self._h, int(granule)), "f5_set_length_buckets")

    def set_isolated_rows(self, on: bool):
        """sample_items() / sample_span() on packed rows, every row as if it were alone in the batch (f5_set_isolated_rows)."""
        _lib.check(self.lib.f5_set_isolated_rows(self._h, int(bool(on))), "f5_set_isolated_rows")

    def set_graph_capacity(self, n: int):
        """The graph cache holds n graphs, 16 <= n <= 64 (f5_set_graph_capacity); set_length_buckets puts it back to 16."""
        _lib.check(self.lib.f5_set_graph_capacity(self._h, int(n)), "f5_set_graph_capacity")

    def prepare_sample(self, batch: int, n_min: int, n_max: int, nt_max: int, steps: int, cfg_strength: float, *,
                       method: str = "euler", want_traj: bool = True):
        """Captures the graphs of every length bucket in [n_min, n_max] ahead of the first request (needs length buckets)."""
        if method not in _lib.ODE_METHODS:
            raise ValueError(f"unknown ODE method {method!r}: expected one of {sorted(_lib.ODE_METHODS)}")
        with torch.cuda.device(self.device):
            _lib.check(self.lib.f5_prepare_sample(self._h, int(batch), int(n_min), int(n_max), int(nt_max), int(steps), float(cfg_strength),
                                                  _lib.ODE_METHODS[method], int(want_traj), _stream_ptr(self.device)),
                       "f5_prepare_sample")

    def graph_stats(self, reset: bool = False) -> dict:
        """sample() bodies captured, replayed and launched eagerly, and graphs evicted, since creation or the last reset."""
        out = (C.c_int32 * 4)()
        _lib.check(self.lib.f5_graph_stats(self._h, out), "f5_graph_stats")
        if reset:
            _lib.check(self.lib.f5_graph_stats(self._h, None), "f5_graph_stats")
        return dict(captures=out[0], replays=out[1], eager=out[2], evictions=out[3])

    # ------------------------------------------------------------------ resident adapters
    def new_adapter(self, pairs: dict, full: dict) -> C.c_void_p:
        """Uploads one adapter: pairs {module: (A [r, in], B [out, r], scale)}, full {name: replacement tensor}.
        Returns the f5_adapter handle (free_adapter)."""
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            st = _stream_ptr(self.device)
            _lib.check(self.lib.f5_adapter_create(self._h, C.byref(h)), "f5_adapter_create")
            try:
                for mod, (a, b, scale) in pairs.items():
                    da, db = _dev_f32(a, self.device), _dev_f32(b, self.device)
                    _lib.check(self.lib.f5_adapter_put_lora(h, (mod + ".weight").encode(), _ptr(da), _lib.shape_array(da.shape), da.dim(),
                                                            _ptr(db), _lib.shape_array(db.shape), db.dim(), float(scale), st),
                               f"f5_adapter_put_lora({mod})")
                for name, t in full.items():
                    d = _dev_f32(t, self.device)
                    _lib.check(self.lib.f5_adapter_put_tensor(h, name.encode(), _ptr(d), _lib.shape_array(d.shape), d.dim(), st),
                               f"f5_adapter_put_tensor({name})")
            except Exception:
                self.lib.f5_adapter_destroy(h)
                raise
        self._adapter_handles.append(h)
        return h

    def free_adapter(self, h):
        _lib.check(self.lib.f5_adapter_destroy(h), "f5_adapter_destroy")
        self._adapter_handles.remove(h)

    def set_adapter(self, h):
        """h: a handle of new_adapter, or None for the base model.  One kernel launch on the current stream."""
        with torch.cuda.device(self.device):
            _lib.check(self.lib.f5_set_adapter(self._h, h, _stream_ptr(self.device)), "f5_set_adapter")

    # ------------------------------------------------------------------ compute
    def text_embed(self, text: torch.Tensor, N: int, lens=None, drop_text=False) -> torch.Tensor:
        B, nt = text.shape
        text = text.to(device=self.device, dtype=torch.long).contiguous()
        out = torch.empty(B, N, self.arch["text_dim"], device=self.device, dtype=torch.float32)
        if self.backbone == "MMDiT":   # the text stream itself: [B, nt, dim], not stretched to N
            out = torch.empty(B, nt, self.arch["dim"], device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.f5_text_embed(self._h, _ptr(text), B, nt, _lib.int_array(lens), N, int(drop_text),
                                              _ptr(out), _stream_ptr(self.device)), "f5_text_embed")
        return out

    def forward(self, x, cond, text, time, lens=None, cfg_infer=False, drop_audio_cond=False, drop_text=False):
        B, N, _ = x.shape
        x = _dev_f32(x, self.device)
        cond = _dev_f32(cond, self.device)
        text = text.to(device=self.device, dtype=torch.long).contiguous()
        tl = [float(v) for v in time] if not isinstance(time, float) else [time] * B
        if len(tl) == 1 and B > 1:
            tl = tl * B
        out = torch.empty((2 * B if cfg_infer else B), N, self.mel_dim, device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.f5_dit_forward(self._h, _ptr(x), _ptr(cond), _ptr(text), text.shape[1],
                                               _lib.float_array(tl), _lib.int_array(lens), B, N, int(cfg_infer),
                                               int(drop_audio_cond), int(drop_text), _ptr(out),
                                               _stream_ptr(self.device)), "f5_dit_forward")
        return out

    def flow_loss(self, x1, x0, text, time, span, lens=None, drop_audio_cond=False, drop_text=False, want_pred=True, want_cond=True,
                  want_frame_err=True):
        """CFM.forward's flow-matching loss around one backbone evaluation (f5_flow_loss): x1 (the mel) and x0 (the noise)
        f32[B, N, mel], text i64[B, nt], time a list of B floats, span a list of B (start, end) frame pairs inside [0, lens[b]].
        Returns (sq_sum f64[B], count i32[B], pred, cond, frame_err), all on the device, the last three None where not wanted.
        Nothing is read back and the host does not wait."""
        B, N, _ = x1.shape
        x1 = _h2d_async(x1, self.device, torch.float32)
        x0 = _h2d_async(x0, self.device, torch.float32)
        text = _h2d_async(text, self.device, torch.long)
        flat = [int(v) for se in span for v in se]
        if len(flat) != 2 * B or len(time) != B:
            raise ValueError(f"flow_loss: {len(time)} times and {len(flat) // 2} spans for a batch of {B}")
        sq_sum = torch.empty(B, device=self.device, dtype=torch.float64)
        count = torch.empty(B, device=self.device, dtype=torch.int32)
        pred = torch.empty(B, N, self.mel_dim, device=self.device, dtype=torch.float32) if want_pred else None
        cond = torch.empty(B, N, self.mel_dim, device=self.device, dtype=torch.float32) if want_cond else None
        frame_err = torch.empty(B, N, device=self.device, dtype=torch.float32) if want_frame_err else None
        with torch.cuda.device(self.device):
            _lib.check(self.lib.f5_flow_loss(self._h, _ptr(x1), _ptr(x0), _ptr(text), text.shape[1], _lib.float_array(time),
                                             _lib.int_array(lens), _lib.int_array(flat), B, N, int(drop_audio_cond), int(drop_text),
                                             _ptr(sq_sum), _ptr(count), _ptr(pred), _ptr(cond), _ptr(frame_err),
                                             _stream_ptr(self.device)), "f5_flow_loss")
        return sq_sum, count, pred, cond, frame_err

    def mmdit_taps(self, buf: torch.Tensor | None):
        """Diagnostic (tests): later forward() calls of an MMDiT engine copy their intermediates into `buf` (f5k_mmdit_taps); None: off."""
        _lib.check(self.lib.f5k_mmdit_taps(self._h, _ptr(buf)), "f5k_mmdit_taps")

    def _stage_call(self, cond, cond_mask, text, B, method):
        """What every sampler call begins with: the method check, cond, cond_mask and text on the device, and `out`.
        Returns (cond, cond_frames, cond_mask, text, out); N is cond_mask's ([B, N])."""
        if method not in _lib.ODE_METHODS:
            raise ValueError(f"unknown ODE method {method!r}: expected one of {sorted(_lib.ODE_METHODS)}")
        cond_frames = 0 if cond is None else cond.shape[1]
        if cond is not None:
            cond = _h2d_async(cond, self.device, torch.float32)
        cm = _h2d_async(cond_mask, self.device, torch.uint8)
        text = _h2d_async(text, self.device, torch.long)
        out = torch.empty(B, cond_mask.shape[1], self.mel_dim, device=self.device, dtype=torch.float32)
        return cond, cond_frames, cm, text, out

    @staticmethod
    def _flat_grids(t_grids):
        """B grids as rows of max(steps) + 1 (the engine ignores what follows an item's own grid): (flat, steps, max(steps))."""
        steps = [len(g) - 1 for g in t_grids]
        flat = []
        for g in t_grids:
            flat += [float(v) for v in g] + [0.0] * (max(steps) + 1 - len(g))
        return flat, steps, max(steps)

    def sample(self, cond, cond_mask, y0, text, t_grid, cfg_strength, lens=None, want_traj=True, method="euler"):
        """cond f32[B,Nc,mel] (Nc <= N: the engine zero-pads, cfm.py:145; None = no_ref_audio), cond_mask bool[B,N],
        y0 f32[B,N,mel], text i64[B,nt], t_grid list[float]; method "euler" (1 backbone evaluation per step) or
        "midpoint" (2 per step), torchdiffeq's fixed-grid solvers on the same grid."""
        B, N, mel = y0.shape
        steps = len(t_grid) - 1
        cond, cond_frames, cm, text, out = self._stage_call(cond, cond_mask, text, B, method)
        y0 = _h2d_async(y0, self.device, torch.float32)
        traj = torch.empty(steps + 1, B, N, mel, device=self.device, dtype=torch.float32) if want_traj else None
        with torch.cuda.device(self.device):
            _lib.check(self.lib.f5_sample_ode(self._h, _ptr(cond), cond_frames, _ptr(cm), _ptr(y0), _ptr(text), text.shape[1],
                                              _lib.float_array(t_grid), steps, float(cfg_strength), _lib.int_array(lens),
                                              B, N, _ptr(out), _ptr(traj), _stream_ptr(self.device), _lib.ODE_METHODS[method]),
                       "f5_sample_ode")
        return out, traj

    def sample_items(self, cond, cond_mask, y0, text, t_grids, cfg_strengths, lens=None, want_traj=True, method="euler"):
        """sample() with per-item settings (f5_sample_items): t_grids a list of B grids (item b makes len(t_grids[b]) - 1 steps),
        cfg_strengths a list of B floats.  The trajectory has max(steps) + 1 slots; an item that has finished keeps its final state."""
        B, N, mel = y0.shape
        if len(t_grids) != B or len(cfg_strengths) != B:
            raise ValueError(f"sample_items: {len(t_grids)} grids and {len(cfg_strengths)} cfg strengths for a batch of {B}")
        cond, cond_frames, cm, text, out = self._stage_call(cond, cond_mask, text, B, method)
        flat, steps, steps_max = self._flat_grids(t_grids)
        y0 = _h2d_async(y0, self.device, torch.float32)
        traj = torch.empty(steps_max + 1, B, N, mel, device=self.device, dtype=torch.float32) if want_traj else None
        with torch.cuda.device(self.device):
            _lib.check(self.lib.f5_sample_items(self._h, _ptr(cond), cond_frames, _ptr(cm), _ptr(y0), _ptr(text), text.shape[1],
                                                _lib.float_array(flat), _lib.int_array(steps), steps_max, _lib.float_array(cfg_strengths),
                                                _lib.int_array(lens), B, N, _ptr(out), _ptr(traj), _stream_ptr(self.device),
                                                _lib.ODE_METHODS[method]), "f5_sample_items")
        return out, traj

    def sample_span(self, cond, cond_mask, y_new, prev_state, rows, text, t_grids, cfg_strengths, lens=None, method="euler"):
        """Some steps of a sample_items solve (f5_sample_span): t_grids a list of B sub-grids (item b makes len(t_grids[b]) - 1 steps
        here), rows[b] the row of prev_state [prev_B, prev_N, mel] item b continues from, or -1 for an item that starts from
        y_new[b] ([B, N, mel]; None when no item starts).  N is cond_mask's ([B, N]).  Returns (out, state), both [B, N, mel]: the
        raw state is the next slice's prev_state."""
        B = len(t_grids)
        rows = [int(r) for r in rows]
        if len(rows) != B or len(cfg_strengths) != B:
            raise ValueError(f"sample_span: {len(rows)} rows and {len(cfg_strengths)} cfg strengths for a batch of {B}")
        N, mel = cond_mask.shape[1], self.mel_dim
        cond, cond_frames, cm, text, out = self._stage_call(cond, cond_mask, text, B, method)
        flat, steps, count = self._flat_grids(t_grids)
        if y_new is not None:
            y_new = _h2d_async(y_new, self.device, torch.float32)
            if tuple(y_new.shape) != (B, N, mel):
                raise ValueError(f"sample_span: y_new is {tuple(y_new.shape)}, not {(B, N, mel)}")
        prev_B = prev_N = 0
        if prev_state is not None:
            prev_state = _h2d_async(prev_state, self.device, torch.float32)
            if prev_state.ndim != 3 or prev_state.shape[2] != mel:
                raise ValueError(f"sample_span: prev_state is {tuple(prev_state.shape)}, not [prev_B, prev_N, {mel}]")
            prev_B, prev_N = prev_state.shape[:2]
        state = torch.empty(B, N, mel, device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.f5_sample_span(self._h, _ptr(cond), cond_frames, _ptr(cm), _ptr(y_new), _ptr(prev_state), prev_B, prev_N,
                                               _lib.int_array(rows), _ptr(text), text.shape[1], _lib.float_array(flat),
                                               _lib.int_array(steps), count, _lib.float_array(cfg_strengths), _lib.int_array(lens), B, N,
                                               _ptr(out), _ptr(state), _stream_ptr(self.device), _lib.ODE_METHODS[method]),
                       "f5_sample_span")
        return out, state

    # ------------------------------------------------------------------ profiling
    def profile(self, on: bool):
        _lib.check(self.lib.f5_profile_enable(self._h, int(on)), "f5_profile_enable")

    def profile_read(self) -> dict:
        n = len(_lib.PROFILE_CLASSES)
        ms = (C.c_float * n)()
        cnt = (C.c_int32 * n)()
        fl = (C.c_double * n)()
        _lib.check(self.lib.f5_profile_read(self._h, ms, cnt, fl, n), "f5_profile_read")
        return {name: dict(ms=ms[i], launches=cnt[i], flops=fl[i]) for i, name in enumerate(_lib.PROFILE_CLASSES)}
