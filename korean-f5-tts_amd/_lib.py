"""ctypes binding of libf5hip.so (include/f5_hip.h).  There is NO fallback: if the library is missing or a call fails
this module raises -- the product path never computes on the CPU or through PyTorch ops."""
from __future__ import annotations

import ctypes as C
import os

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libf5hip.so")

F5_OPT_QK_RMSNORM, F5_OPT_LONG_SKIP, F5_OPT_TEXT_AVG_UPSAMPLE, F5_OPT_ADAPTERS = 1, 2, 4, 8
F5_PREC_F32, F5_PREC_BF16, F5_PREC_F16, F5_PREC_F16X3, F5_PREC_F16P, F5_PREC_F8 = 0, 1, 2, 3, 4, 5
PRECISIONS = {"f32": F5_PREC_F32, "fp32": F5_PREC_F32, "bf16": F5_PREC_BF16, "f16": F5_PREC_F16, "fp16": F5_PREC_F16,
              "f16x3": F5_PREC_F16X3, "f16p": F5_PREC_F16P, "parity": F5_PREC_F16P, "f8": F5_PREC_F8, "fp8": F5_PREC_F8}
F5_BACKBONE_DIT, F5_BACKBONE_UNETT, F5_BACKBONE_MMDIT = 0, 1, 2
BACKBONES = {"DiT": F5_BACKBONE_DIT, "UNetT": F5_BACKBONE_UNETT, "MMDiT": F5_BACKBONE_MMDIT}
F5_ODE_EULER, F5_ODE_MIDPOINT = 0, 1
ODE_METHODS = {"euler": F5_ODE_EULER, "midpoint": F5_ODE_MIDPOINT}
F5_PCM_F32, F5_PCM_S16 = 0, 1
PCM_FORMATS = {"f32": F5_PCM_F32, "s16": F5_PCM_S16}
ACT_NONE, ACT_GELU_TANH, ACT_GELU_ERF, ACT_SILU, ACT_MISH = 0, 1, 2, 3, 4
PROFILE_CLASSES = ("gemm", "attention", "layernorm", "convpos", "misc", "text_encoder", "time_adaln")


class F5Error(RuntimeError):
    pass


class f5_config(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "backbone", "precision", "dim", "depth", "heads", "dim_head", "ff_dim", "text_dim", "conv_layers",
        "pe_attn_head", "text_mask_padding", "attn_mask_enabled", "text_num_embeds", "mel_dim", "max_pos", "options")] + \
        [("reserved", C.c_int32 * 4)]


class f5_bigvgan_config(C.Structure):
    _fields_ = [("num_mels", C.c_int32), ("upsample_initial_channel", C.c_int32), ("num_upsamples", C.c_int32),
                ("upsample_rates", C.c_int32 * 8), ("upsample_kernel_sizes", C.c_int32 * 8), ("num_kernels", C.c_int32),
                ("resblock_kernel_sizes", C.c_int32 * 4), ("num_dilations", C.c_int32), ("resblock_dilations", C.c_int32 * 4),
                ("use_tanh_at_final", C.c_int32), ("use_bias_at_final", C.c_int32), ("precision", C.c_int32),
                ("reserved", C.c_int32 * 3)]


class f5_vocos_config(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("input_channels", "dim", "intermediate_dim", "num_layers", "n_fft",
                                         "hop_length")] + [("reserved", C.c_int32 * 4)]


_p = C.c_void_p
_i = C.c_int32
_f = C.c_float

F5K_EPI_STORE, F5K_EPI_GATE_RES, F5K_EPI_QKV, F5K_EPI_QKNORM = 0, 1, 2, 3
# the buffers of f5k_work_plan, in its order (F5K_WORK_NAMES of include/f5_hip.h)
F5K_WORK_NAMES = ("tdev feat th temb st mod lens lens_plain row_start rowmap step_cond text_c text_u tx_a tx_b tx_h1 grn_part uc acat h c1 x "
                  "pred xn q k ao vt ffh a8 a8s in_cond y y_mid out_buf traj_buf in_mask in_text cat2 skips pred_all mod_rows it_t it_cfg it_steps "
                  "it_idx").split()


class f5k_epi(C.Structure):
    """Epilogue parameters of f5k_gemm_epi (include/f5_hip.h)."""
    _fields_ = [(n, C.c_int32) for n in ("kind", "cfg", "a_presplit", "m_limit", "out16", "act", "planar", "gate_stride",
                                         "rows_per_batch", "nlens")] + \
        [("res", _p), ("gate", _p), ("lens_host", C.POINTER(C.c_int32))] + \
        [(n, C.c_int32) for n in ("H", "Nseq", "Npad", "pe_heads")] + [("q_scale", C.c_float), ("maxpos", C.c_int32)] + \
        [("rope_cos", _p), ("rope_sin", _p), ("row_start_host", C.POINTER(C.c_int32)), ("Bp", C.c_int32), ("pad0", C.c_int32),
         ("gq", _p), ("gk", _p), ("out0", _p), ("out1", _p), ("out2", _p), ("out0_f32", _p), ("out1_f32", _p), ("out2_f32", _p),
         ("n0", C.c_int64), ("n1", C.c_int64), ("n2", C.c_int64)]

class f5k_attn(C.Structure):
    """Launch-form parameters of f5k_attention_ex (include/f5_hip.h)."""
    _fields_ = [("kv_lens_host", C.POINTER(C.c_int32)), ("q_lens_host", C.POINTER(C.c_int32)), ("row_start_host", C.POINTER(C.c_int32)),
                ("nlens", C.c_int32), ("mode", C.c_int32), ("hi_only", C.c_int32), ("o_planar", C.c_int32), ("vt_pad_fill", C.c_float),
                ("pad0", C.c_int32), ("out", _p), ("out_f32", _p), ("n_out", C.c_int64)]


class f5k_conv(C.Structure):
    """Launch-form parameters of f5k_convpos_ex (include/f5_hip.h)."""
    _fields_ = [("lens_host", C.POINTER(C.c_int32)), ("row_start_host", C.POINTER(C.c_int32)), ("nlens", C.c_int32), ("pad0", C.c_int32),
                ("rows", C.c_int64)]


# name -> (restype, argtypes); mirrors include/f5_hip.h exactly (tests/test_abi.py checks the export list)
SIGNATURES = {
    "f5_last_error": (C.c_char_p, []),
    "f5_version": (C.c_char_p, []),
    "f5_create": (_i, [C.POINTER(f5_config), C.POINTER(_p)]),
    "f5_destroy": (_i, [_p]),
    "f5_load_weight": (_i, [_p, C.c_char_p, _p, C.POINTER(C.c_int64), _i, _p]),
    "f5_finalize": (_i, [_p, _p]),
    "f5_text_embed": (_i, [_p, _p, _i, _i, C.POINTER(_i), _i, _i, _p, _p]),
    "f5_dit_forward": (_i, [_p, _p, _p, _p, _i, C.POINTER(_f), C.POINTER(_i), _i, _i, _i, _i, _i, _p, _p]),
    "f5_flow_loss": (_i, [_p, _p, _p, _p, _i, C.POINTER(_f), C.POINTER(_i), C.POINTER(_i), _i, _i, _i, _i, _p, _p, _p, _p, _p, _p]),
    "f5_sample": (_i, [_p, _p, _i, _p, _p, _p, _i, C.POINTER(_f), _i, _f, C.POINTER(_i), _i, _i, _p, _p, _p]),
    "f5_sample_ode": (_i, [_p, _p, _i, _p, _p, _p, _i, C.POINTER(_f), _i, _f, C.POINTER(_i), _i, _i, _p, _p, _p, _i]),
    "f5_sample_items": (_i, [_p, _p, _i, _p, _p, _p, _i, C.POINTER(_f), C.POINTER(_i), _i, C.POINTER(_f), C.POINTER(_i), _i, _i, _p, _p,
                             _p, _i]),
    "f5_sample_span": (_i, [_p, _p, _i, _p, _p, _p, _i, _i, C.POINTER(_i), _p, _i, C.POINTER(_f), C.POINTER(_i), _i, C.POINTER(_f),
                            C.POINTER(_i), _i, _i, _p, _p, _p, _i]),
    "f5_reserve": (_i, [_p, _i, _i, _i]),
    "f5_set_length_buckets": (_i, [_p, _i]),
    "f5_set_isolated_rows": (_i, [_p, _i]),
    "f5_set_graph_capacity": (_i, [_p, _i]),
    "f5_prepare_sample": (_i, [_p, _i, _i, _i, _i, _i, _f, _i, _i, _p]),
    "f5_graph_stats": (_i, [_p, C.POINTER(_i)]),
    "f5_adapter_create": (_i, [_p, C.POINTER(_p)]),
    "f5_adapter_destroy": (_i, [_p]),
    "f5_adapter_put_lora": (_i, [_p, C.c_char_p, _p, C.POINTER(C.c_int64), _i, _p, C.POINTER(C.c_int64), _i, _f, _p]),
    "f5_adapter_put_tensor": (_i, [_p, C.c_char_p, _p, C.POINTER(C.c_int64), _i, _p]),
    "f5_set_adapter": (_i, [_p, _p, _p]),
    "f5_vocos_create": (_i, [C.POINTER(f5_vocos_config), C.POINTER(_p)]),
    "f5_vocos_destroy": (_i, [_p]),
    "f5_vocos_load_weight": (_i, [_p, C.c_char_p, _p, C.POINTER(C.c_int64), _i, _p]),
    "f5_vocos_finalize": (_i, [_p, _p]),
    "f5_vocos_decode": (_i, [_p, _p, _i, _i, _p, _p]),
    "f5_vocos_decode_strided": (_i, [_p, _p, _i, _i, C.c_int64, C.c_int64, C.c_int64, _p, _p]),
    "f5_vocos_decode_ragged": (_i, [_p, _p, _i, C.c_int64, C.c_int64, C.c_int64, C.POINTER(_i), C.POINTER(_i), C.POINTER(_f), _p,
                               C.c_int64, _p]),
    "f5_wave_crossfade": (_i, [_p, _i, C.c_int64, C.POINTER(_i), _i, _p, C.c_int64, C.POINTER(C.c_int64), _p]),
    "f5_wave_join": (_i, [_p, _i, C.POINTER(C.c_int64), C.POINTER(_i), C.POINTER(_i), _p, C.c_int64, C.POINTER(C.c_int64), _p]),
    "f5_edit_assemble": (_i, [_p, _i, C.c_int64, _i, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), _p, _i, _p]),
    "f5_wave_splice": (_i, [_p, _i, C.c_int64, C.POINTER(_i), _p, C.POINTER(C.c_int64), C.POINTER(_i), C.POINTER(_i), C.POINTER(_i),
                        _i, _i, _p, C.c_int64, _p]),
    "f5_silence_plan": (_i, [_i, C.POINTER(_i), _i, C.POINTER(_i), C.POINTER(_i), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "f5_silence_analyse": (_i, [_p, _i, C.POINTER(C.c_int64), C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), _f, _i,
                                C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), _p, C.c_int64, _p]),
    "f5_wave_gather": (_i, [_p, _i, C.POINTER(C.c_int64), C.POINTER(_i), C.POINTER(_i), _f, C.POINTER(_i), C.POINTER(_i),
                            C.POINTER(_i), C.POINTER(C.c_int64), _p, C.c_int64, _p]),
    "f5_mel_distance_plan": (_i, [_i, C.POINTER(_i), C.POINTER(_i), _i, C.POINTER(_i), C.POINTER(C.c_int64)]),
    "f5_mel_distance": (_i, [_p, _p, _i, C.POINTER(C.c_int64), C.POINTER(_i), C.c_int64, C.POINTER(C.c_int64), C.POINTER(_i), C.c_int64,
                             _i, _i, _p, _p]),
    "f5_mel_align_plan": (_i, [_i, C.POINTER(_i), C.POINTER(_i), _i, C.POINTER(_i), C.POINTER(C.c_int64)]),
    "f5_mel_align": (_i, [_p, _p, _i, C.POINTER(C.c_int64), C.POINTER(_i), C.c_int64, C.POINTER(C.c_int64), C.POINTER(_i), C.c_int64,
                          _i, _i, _p, _p, _p, _p]),
    "f5_pitch_track": (_i, [_p, _i, C.POINTER(C.c_int64), C.POINTER(_i), _i, _i, _i, C.POINTER(_i), _i, _i, _i, C.c_double, _p, _p,
                            _p]),
    "f5_pitch_candidates": (_i, [_p, _i, C.POINTER(C.c_int64), C.POINTER(_i), _i, _i, _i, C.POINTER(_i), _i, _i, _i, _i,
                                 C.POINTER(C.c_double), C.c_double, _p, _p, _p, _p, _p]),
    "f5_pitch_decode_bytes": (C.c_int64, [C.c_int64, _i]),
    "f5_pitch_decode": (_i, [_p, _p, _p, _i, _i, C.POINTER(_i), _i, C.POINTER(C.c_double), C.POINTER(C.c_double), _i,
                             C.POINTER(C.c_double), C.c_double, _p, C.c_int64, _p, _p, _p]),
    "f5_cep_moments_plan": (_i, [_i, C.POINTER(_i), _i, _i, C.POINTER(C.c_int64)]),
    "f5_cep_moments": (_i, [_p, _i, C.POINTER(C.c_int64), C.POINTER(_i), C.c_int64, _i, _i, _i, _p, C.c_double, _p, _p, _p, _p]),
    "f5_gauss_divergence": (_i, [_p, _p, _p, _i, _p, _p, _p, _i, _i, _i, C.POINTER(_i), C.POINTER(_i), _p, _p, _p]),
    "f5_bigvgan_create": (_i, [C.POINTER(f5_bigvgan_config), C.POINTER(_p)]),
    "f5_bigvgan_destroy": (_i, [_p]),
    "f5_bigvgan_load_weight": (_i, [_p, C.c_char_p, _p, C.POINTER(C.c_int64), _i, _p]),
    "f5_bigvgan_finalize": (_i, [_p, _p]),
    "f5_bigvgan_forward": (_i, [_p, _p, _i, _i, C.c_int64, C.c_int64, C.c_int64, _p, _p]),
    "f5_bigvgan_forward_ragged": (_i, [_p, _p, _i, C.c_int64, C.c_int64, C.c_int64, C.POINTER(_i), C.POINTER(_i), C.POINTER(_f), _p,
                                  C.c_int64, _p]),
    "f5_bigvgan_ragged_plan": (_i, [C.POINTER(f5_bigvgan_config), _i, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)]),
    "f5_mel_create": (_i, [_i, _i, _i, C.POINTER(_p)]),
    "f5_mel_destroy": (_i, [_p]),
    "f5_mel_load": (_i, [_p, C.c_char_p, _p, C.POINTER(C.c_int64), _i, _p]),
    "f5_mel_forward": (_i, [_p, _p, _i, _i, _p, _p]),
    "f5_mel_forward_ex": (_i, [_p, _p, _i, _i, _i, _f, _p, _p]),
    "f5_mel_ragged_plan": (_i, [_i, _i, _i, _i, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)]),
    "f5_mel_forward_ragged": (_i, [_p, _p, _i, C.POINTER(C.c_int64), C.POINTER(_i), _i, _f, _p, C.c_int64, _i, _p]),
    "f5_mel_prepare_plan": (_i, [_i, C.POINTER(_i), C.POINTER(_i), _i, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                            C.POINTER(C.c_int64)]),
    "f5_mel_resample_bank": (_i, [_p, _i, _i, _p, C.c_int64, _p]),
    "f5_mel_resample_bank_count": (_i, [_p, C.POINTER(_i)]),
    "f5_mel_prepare_ragged": (_i, [_p, _p, _i, C.POINTER(C.c_int64), C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), _i, _f, _p,
                              C.c_int64, _p, _p]),
    "f5_wave_deliver_plan": (_i, [_i, C.c_int64, _i, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "f5_wave_deliver": (_i, [_p, _p, _i, C.POINTER(C.c_int64), C.POINTER(_i), C.POINTER(_i), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                             _i, _i, _p, C.c_int64, C.POINTER(C.c_int64), _p]),
    "f5_wave_emit": (_i, [_p, _p, _i, C.POINTER(_i), C.POINTER(C.c_int64), C.POINTER(_i), C.POINTER(_i), C.POINTER(C.c_int64),
                          C.POINTER(_i), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(_i), C.POINTER(_i), _p, C.c_int64,
                          C.POINTER(C.c_int64), _p]),
    "f5k_gemm": (_i, [_i, _p, _p, _p, _i, _p, _i, _i, _i, _i, _i, _p]),
    "f5k_gemm_plan": (_i, [_i] * 12 + [C.POINTER(_i)]),
    "f5k_attention": (_i, [_i, _p, _p, _p, C.POINTER(_i), _p, _i, _i, _i, _p]),
    "f5k_convpos": (_i, [_i, _p, _p, _p, _p, C.POINTER(_i), _p, _i, _i, _i, _p]),
    "f5k_attention_ex": (_i, [_i, _p, _p, _p, _i, _i, _i, C.POINTER(f5k_attn), _p]),
    "f5k_convpos_ex": (_i, [_i, _p, _p, _p, _p, _p, _i, _i, _i, C.POINTER(f5k_conv), _p]),
    "f5k_layernorm_mod": (_i, [_p, _p, _p, _p, _i, _i, _i, _f, _p]),
    "f5k_layernorm_mod_ex": (_i, [_i, _p, _p, _p, _p, _p, _i, _i, _i, _f, _i, _i, _p]),
    "f5k_layernorm_q8": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _f, _i, C.POINTER(_i), _p]),
    "f5k_quant_rows_e4m3": (_i, [_i, _p, C.c_int64, _i, _i, _p, C.c_int64, _p, _i, _p]),
    "f5k_gemm_epi": (_i, [_i, _p, _p, _p, _i, _i, _i, C.POINTER(f5k_epi), _p]),
    "f5k_pack_input": (_i, [_i, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _p, _p, _p, _p]),
    "f5k_fill_rowmap": (_i, [_p, _p, _i, _p]),
    "f5k_euler_cfg": (_i, [_p, _p, _i, _i, _i, _p, _p, _p, _i, _f, _i, _p, _p]),
    "f5k_midpoint_half_cfg": (_i, [_p, _p, _i, _i, _i, _p, _p, _p, _i, _f, _i, _p, _p]),
    "f5k_euler_cfg_items": (_i, [_p, _p, _i, _i, _i, _p, _p, _p, _i, _i, _i, _p, _p]),
    "f5k_midpoint_half_cfg_items": (_i, [_p, _p, _i, _i, _i, _p, _p, _p, _i, _i, _i, _p, _p]),
    "f5k_euler_cfg_items_packed": (_i, [_p, _p, _i, _i, _i, _p, _p, _p, _p, _p, _i, _i, _i, _p, _p]),
    "f5k_midpoint_half_cfg_items_packed": (_i, [_p, _p, _i, _i, _i, _p, _p, _p, _p, _p, _i, _i, _i, _p, _p]),
    "f5k_flow_mix": (_i, [_p, _p, _p, _p, C.POINTER(_i), _p, _p, _i, _i, _i, _p]),
    "f5k_flow_loss_reduce": (_i, [_p, _p, _p, _p, C.POINTER(_i), _p, _p, _p, _p, _i, _i, _i, _p]),
    "f5k_mod_gather": (_i, [_p, _p, _p, _i, _i, _i, _p]),
    "f5k_span_stage": (_i, [_p, _p, _i, _i, _p, _p, C.POINTER(_i), _i, _i, _i, _p]),
    "f5k_span_stage_pitched": (_i, [_p, _i, _p, _i, _i, _p, _p, C.POINTER(_i), _i, _i, _i, _p]),
    "f5k_item_time_rows": (_i, [C.POINTER(_f), C.POINTER(_i), _i, _i, _i, C.POINTER(_f), C.POINTER(_i), C.POINTER(_i)]),
    "f5k_select_rows": (_i, [_p, _p, _p, _p, C.c_int64, _i, _p]),
    "f5k_time_sinus": (_i, [_p, _p, _p, _i, _p]),
    "f5k_xrmsnorm": (_i, [_i, _p, _p, _i, _i, _p, _i, _p]),
    "f5k_unett_assemble": (_i, [_p, _p, _i, _p, _i, _i, _i, _p]),
    "f5k_cat2": (_i, [_i, _p, _p, _p, _i, _i, _i, _p]),
    "f5k_strip_first_token": (_i, [_p, _p, _i, _i, _i, _p]),
    "f5k_work_plan": (_i, [C.POINTER(f5_config), _i, _i, _i, _i, _i, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "f5k_mmdit_taps": (_i, [_p, _p]),
    "f5k_gemm_time": (_i, [_i, _i, _i, _i, _i, _i, _i, C.POINTER(_f), _p]),
    "f5_profile_enable": (_i, [_p, _i]),
    "f5_profile_read": (_i, [_p, C.POINTER(_f), C.POINTER(_i), C.POINTER(C.c_double), _i]),
}

_lib = None


def load() -> C.CDLL:
    """Loads the engine library; raises F5Error (never falls back) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise F5Error(f"{LIB_PATH} is missing: build it with `python korean-f5-tts_amd/build.py` "
                      "(or __graft_entry__.build()); there is no CPU / PyTorch fallback for the F5-TTS hot path")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = load().f5_last_error().decode(errors="replace")
        raise F5Error(f"{what or 'libf5hip'} failed (code {rc}): {msg}")


def int_array(vals):
    if vals is None:
        return None
    return (C.c_int32 * len(vals))(*[int(v) for v in vals])


def float_array(vals):
    return (C.c_float * len(vals))(*[float(v) for v in vals])


def shape_array(shape):
    return (C.c_int64 * max(len(shape), 1))(*[int(s) for s in shape])


def _stream_ptr(device) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _ptr(t: torch.Tensor | None) -> C.c_void_p:
    return C.c_void_p(0 if t is None else t.data_ptr())


def _dev_f32(t: torch.Tensor, device) -> torch.Tensor:
    return t.detach().to(device=device, dtype=torch.float32).contiguous()
