"""ctypes binding of libvvtts_hip.so (include/vvtts.h) and the device-resident synthesis driver.

PyTorch is used only as plumbing here: it owns HBM tensors, the HIP stream and (multi-GPU) the
RCCL broadcast.  Every arithmetic step of the hot path runs in the hand-written gfx950 kernels
behind the C ABI.  There is NO CPU fallback: if the library or a GPU is missing this module
raises, loudly (the oracle under oracle/ is test infrastructure and is never imported here).
"""
from __future__ import annotations

import ctypes as C
import os
import contextlib
import threading
from typing import Dict, Optional, Tuple

import torch

from . import pack
from .model_spec import (ODE_MAX_EVALS, ODE_MULTISTEP, ModelSpec, block_cache_schedule, check_apg, check_block_cache, check_cfg_norm, guidance_mask,
                         ode_plan)
from .pcm_stage import JOIN_MAX_N, LOUD_RUN, PcmStage, _ptr, plan_join  # noqa: F401  (the constants and plan_join stay importable from here)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VVTTS_LIB") or os.path.join(_HERE, "libvvtts_hip.so")   # VVTTS_LIB: A/B builds in tools/

VV_F32, VV_BF16 = 0, 1
PROF_CLASSES = ["gemm", "attention", "norm", "posconv", "elementwise", "voc_conv", "voc_post", "mel", "text",
                "voc_pre", "voc_up0", "voc_up1", "voc_up2", "voc_up3", "voc_mrf0", "voc_mrf1", "voc_mrf2", "voc_mrf3"]   # voc_conv once more, by stage


class HipUnavailable(RuntimeError):
    pass


class vv_model_cfg(C.Structure):
    _fields_ = [
        ("n_mel", C.c_int32), ("n_fft", C.c_int32), ("win_length", C.c_int32), ("hop_length", C.c_int32),
        ("dim", C.c_int32), ("depth", C.c_int32), ("heads", C.c_int32), ("head_dim", C.c_int32), ("ff_mult", C.c_int32),
        ("text_dim", C.c_int32), ("text_layers", C.c_int32), ("text_conv_k", C.c_int32), ("text_ff_mult", C.c_int32),
        ("vocab_rows", C.c_int32), ("pos_conv_k", C.c_int32), ("pos_conv_groups", C.c_int32), ("time_freq_dim", C.c_int32),
        ("cfg_strength", C.c_float),
        ("voc_pre_ch", C.c_int32), ("voc_pre_k", C.c_int32), ("voc_post_k", C.c_int32),
        ("voc_n_up", C.c_int32), ("voc_up_rates", C.c_int32 * 8), ("voc_up_kernels", C.c_int32 * 8),
        ("voc_n_res", C.c_int32), ("voc_res_kernels", C.c_int32 * 4),
        ("voc_n_dil", C.c_int32), ("voc_res_dilations", C.c_int32 * 4),
        ("voc_lrelu", C.c_float), ("max_pos", C.c_int32),
    ]


class vv_vocos_cfg(C.Structure):
    _fields_ = [("dim", C.c_int32), ("intermediate", C.c_int32), ("layers", C.c_int32), ("embed_k", C.c_int32), ("dw_k", C.c_int32),
                ("ln_eps", C.c_float), ("n_fft", C.c_int32), ("win_length", C.c_int32), ("hop_length", C.c_int32)]


class vv_gemm_args(C.Structure):
    _fields_ = [("dtype", C.c_int32), ("out_dtype", C.c_int32), ("mode", C.c_int32), ("act", C.c_int32),
                ("A", C.c_void_p), ("lda", C.c_int32), ("W", C.c_void_p), ("ldw", C.c_int32), ("C", C.c_void_p), ("ldc", C.c_int32),
                ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32),
                ("bias", C.c_void_p), ("gate", C.c_void_p), ("cos_q", C.c_void_p), ("sin_q", C.c_void_p),
                ("cos_k", C.c_void_p), ("sin_k", C.c_void_p),
                ("n_store", C.c_int32), ("seq_n", C.c_int32), ("rope_dim", C.c_int32),
                ("rope_cs_q", C.c_void_p), ("rope_cs_k", C.c_void_p), ("tile", C.c_int32), ("rope_pos", C.c_void_p), ("rope_by_row", C.c_int32),
                ("tail_parts", C.c_int32), ("tail_row0", C.c_int32), ("C_tail", C.c_void_p), ("rope_theta", C.c_float), ("rope_skip_q", C.c_int32), ("chip_share", C.c_int32)]


class vv_attn_args(C.Structure):
    _fields_ = [("dtype", C.c_int32), ("qkv", C.c_void_p), ("ld_qkv", C.c_int32), ("out", C.c_void_p), ("ld_out", C.c_int32),
                ("n_seq", C.c_int32), ("seq_n", C.c_int32), ("heads", C.c_int32), ("dim", C.c_int32), ("kv_len", C.c_void_p),
                ("row_start", C.c_void_p), ("total_rows", C.c_int32), ("q_scale", C.c_float), ("rope_cs_q", C.c_void_p)]


class vv_ln_args(C.Structure):
    _fields_ = [("out_dtype", C.c_int32), ("x", C.c_void_p), ("ldx", C.c_int32), ("y", C.c_void_p), ("ldy", C.c_int32),
                ("R", C.c_int32), ("D", C.c_int32), ("w", C.c_void_p), ("b", C.c_void_p), ("add_one", C.c_int32), ("eps", C.c_float),
                ("delta", C.c_void_p), ("delta_dtype", C.c_int32), ("ld_delta", C.c_int32),
                ("delta2", C.c_void_p), ("keep_x", C.c_int32), ("tail_row0", C.c_int32), ("delta_tail_parts", C.c_int32),
                ("delta2_tail_parts", C.c_int32), ("delta_tail", C.c_void_p), ("delta2_tail", C.c_void_p)]


class vv_posconv_args(C.Structure):
    _fields_ = [("dtype", C.c_int32), ("out_dtype", C.c_int32), ("in_", C.c_void_p), ("ld_in", C.c_int32), ("W", C.c_void_p),
                ("bias", C.c_void_p), ("out", C.c_void_p), ("ld_out", C.c_int32), ("resid", C.c_void_p), ("ld_resid", C.c_int32),
                ("n_seq", C.c_int32), ("seq_n", C.c_int32), ("groups", C.c_int32), ("KW", C.c_int32), ("B", C.c_int32),
                ("seq_len", C.c_void_p), ("row_start", C.c_void_p)]


class vv_conv_args(C.Structure):
    _fields_ = [("in_", C.c_void_p), ("W", C.c_void_p), ("bias", C.c_void_p), ("out", C.c_void_p), ("resid", C.c_void_p),
                ("B", C.c_int32), ("Cin", C.c_int32), ("Cout", C.c_int32), ("T_in", C.c_int32), ("T_out", C.c_int32),
                ("KW", C.c_int32), ("dil", C.c_int32), ("transposed", C.c_int32), ("up", C.c_int32),
                ("rows_total", C.c_int32), ("rows_pad", C.c_int32), ("accumulate", C.c_int32),
                ("pre_slope", C.c_float), ("out_scale", C.c_float), ("len_in", C.c_void_p), ("W_x3", C.c_void_p), ("wg_rows", C.c_int32)]


class vv_mrf_args(C.Structure):
    _fields_ = [("y", C.c_void_p), ("W1", C.c_void_p), ("b1", C.c_void_p), ("W2", C.c_void_p), ("b2", C.c_void_p), ("out", C.c_void_p),
                ("B", C.c_int32), ("C", C.c_int32), ("T", C.c_int32), ("KW", C.c_int32), ("dil", C.c_int32), ("rows_pad", C.c_int32),
                ("accumulate", C.c_int32), ("slope", C.c_float), ("out_scale", C.c_float), ("len_in", C.c_void_p)]


class vv_steps_args(C.Structure):
    _fields_ = [("B", C.c_int32), ("N", C.c_int32), ("seq_len", C.c_void_p), ("seq_len_host", C.c_void_p), ("x", C.c_void_p),
                ("cat_mel_text", C.c_void_p), ("cat_mel_text_drop", C.c_void_p), ("rope_cos_q", C.c_void_p), ("rope_sin_q", C.c_void_p),
                ("rope_cos_k", C.c_void_p), ("rope_sin_k", C.c_void_p), ("step0", C.c_int32), ("n_steps", C.c_int32),
                ("ws", C.c_void_p), ("ws_bytes", C.c_uint64), ("cfg_item", C.c_void_p)]


class vv_ode_stage_args(C.Structure):
    _fields_ = [("x", C.c_void_p), ("pred", C.c_void_p), ("ldp", C.c_int32), ("Rc", C.c_int32), ("n_mel", C.c_int32), ("n_prev", C.c_int32),
                ("k_prev", C.c_void_p * 3), ("coef", C.c_float * 4), ("k_out", C.c_void_p), ("x_out", C.c_void_p),
                ("g", C.c_float), ("g_item", C.c_void_p), ("seq_n", C.c_int32), ("row_src", C.c_void_p)]


class vv_apg_args(C.Structure):
    _fields_ = [("eta", C.c_void_p), ("norm_rms", C.c_void_p), ("t_host", C.c_void_p)]


class vv_apg_coef_args(C.Structure):
    _fields_ = [("pred", C.c_void_p), ("ldp", C.c_int32), ("Rc", C.c_int32), ("n_mel", C.c_int32), ("u_row", C.c_void_p),
                ("x_e", C.c_void_p), ("row_src", C.c_void_p), ("B", C.c_int32), ("n_tiles", C.c_int32), ("row_start", C.c_void_p),
                ("len", C.c_void_p), ("t_e", C.c_float), ("g", C.c_float), ("g_item", C.c_void_p), ("eta", C.c_void_p),
                ("norm_rms", C.c_void_p), ("partials", C.c_void_p), ("coef", C.c_void_p)]


class vv_apg_stage_args(C.Structure):
    _fields_ = [("coef", C.c_void_p), ("x_e", C.c_void_p), ("x_e_packed", C.c_int32), ("t_e", C.c_float)]


class vv_cfg_norm_args(C.Structure):
    _fields_ = [("star", C.c_void_p), ("rescale", C.c_void_p), ("report", C.c_void_p)]


class vv_cfg_norm_coef_args(C.Structure):
    _fields_ = [("pred", C.c_void_p), ("ldp", C.c_int32), ("Rc", C.c_int32), ("n_mel", C.c_int32), ("u_row", C.c_void_p),
                ("B", C.c_int32), ("n_tiles", C.c_int32), ("row_start", C.c_void_p), ("len", C.c_void_p), ("g", C.c_float),
                ("g_item", C.c_void_p), ("star", C.c_void_p), ("rescale", C.c_void_p), ("partials", C.c_void_p), ("coef", C.c_void_p),
                ("report", C.c_void_p)]


class vv_ode_diff_args(C.Structure):
    _fields_ = [("f", C.c_void_p), ("f_prev", C.c_void_p), ("Rc", C.c_int32), ("n_mel", C.c_int32), ("B", C.c_int32), ("n_tiles", C.c_int32),
                ("row_start", C.c_void_p), ("len", C.c_void_p), ("partials", C.c_void_p), ("report", C.c_void_p)]


class vv_reuse_args(C.Structure):
    _fields_ = [("report", C.c_void_p), ("report_B", C.c_int32), ("report_evals", C.c_int32)]


class vv_reuse_stage_args(C.Structure):
    _fields_ = [("d_buf", C.c_void_p), ("item_mode_host", C.c_void_p), ("n_items", C.c_int32)]


class vv_cfg_drift_args(C.Structure):
    _fields_ = [("pred", C.c_void_p), ("ldp", C.c_int32), ("Rc", C.c_int32), ("n_mel", C.c_int32), ("u_row", C.c_void_p),
                ("d_buf", C.c_void_p), ("has_old_host", C.c_void_p), ("B", C.c_int32), ("n_tiles", C.c_int32),
                ("row_start", C.c_void_p), ("len", C.c_void_p), ("partials", C.c_void_p), ("report", C.c_void_p)]


class vv_block_cache_args(C.Structure):
    _fields_ = [("first", C.c_int32), ("last", C.c_int32), ("modes_host", C.c_void_p), ("n_modes", C.c_int32), ("report", C.c_void_p),
                ("report_B", C.c_int32), ("report_evals", C.c_int32)]


class vv_block_span_args(C.Structure):
    _fields_ = [("mode", C.c_int32), ("delta_dtype", C.c_int32), ("x", C.c_void_p), ("d1", C.c_void_p), ("d2", C.c_void_p), ("buf", C.c_void_p),
                ("R", C.c_int32), ("D", C.c_int32)]


class vv_block_drift_args(C.Structure):
    _fields_ = [("d_new", C.c_void_p), ("d_prev", C.c_void_p), ("R", C.c_int32), ("D", C.c_int32), ("n_seq", C.c_int32), ("n_items", C.c_int32),
                ("branch0", C.c_int32), ("n_tiles", C.c_int32), ("row_start", C.c_void_p), ("len", C.c_void_p), ("partials", C.c_void_p),
                ("report", C.c_void_p)]


SPAN_MARK, SPAN_DIFF, SPAN_APPLY = 0, 1, 2      # VV_SPAN_* of include/vvtts.h: the form of one vv_block_span launch (N23)

REUSE_LOAD, REUSE_STORE = 1, 2          # VV_REUSE_LOAD / VV_REUSE_STORE of include/vvtts.h: an item's mode in vv_ode_stage_reuse

APG_TILE = 32                 # VV_APG_TILE of include/vvtts.h: frames per partial sum of the projected-guidance reduction

EXPORTS = {
    # name: (restype, argtypes)
    "vv_version": (C.c_char_p, []),
    "vv_last_error": (C.c_char_p, [C.c_void_p]),
    "vv_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.POINTER(vv_model_cfg), C.c_int]),
    "vv_destroy": (None, [C.c_void_p]),
    "vv_bind_weight": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_uint64]),
    "vv_finalize_weights": (C.c_int, [C.c_void_p]),
    "vv_set_time_grid": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "vv_set_ode_plan": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vv_set_ode_multistep": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "vv_set_ode_report": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "vv_ode_diff_reduce": (C.c_int, [C.c_void_p, C.POINTER(vv_ode_diff_args), C.c_void_p]),
    "vv_transformer_steps_ex": (C.c_int, [C.c_void_p, C.POINTER(vv_steps_args), C.c_void_p]),
    "vv_ode_stage": (C.c_int, [C.c_void_p, C.POINTER(vv_ode_stage_args), C.c_void_p]),
    "vv_transformer_steps_guided": (C.c_int, [C.c_void_p, C.POINTER(vv_steps_args), C.c_void_p, C.c_int, C.c_void_p]),
    "vv_transformer_guided_ws_bytes": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_uint64)]),
    "vv_ode_stage_guided": (C.c_int, [C.c_void_p, C.POINTER(vv_ode_stage_args), C.c_void_p, C.c_void_p]),
    "vv_transformer_steps_apg": (C.c_int, [C.c_void_p, C.POINTER(vv_steps_args), C.c_void_p, C.c_int, C.POINTER(vv_apg_args), C.c_void_p]),
    "vv_transformer_apg_ws_bytes": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_uint64)]),
    "vv_apg_coef": (C.c_int, [C.c_void_p, C.POINTER(vv_apg_coef_args), C.c_void_p]),
    "vv_ode_stage_apg": (C.c_int, [C.c_void_p, C.POINTER(vv_ode_stage_args), C.c_void_p, C.POINTER(vv_apg_stage_args), C.c_void_p]),
    "vv_transformer_steps_norm": (C.c_int, [C.c_void_p, C.POINTER(vv_steps_args), C.c_void_p, C.c_int, C.POINTER(vv_cfg_norm_args), C.c_void_p]),
    "vv_transformer_norm_ws_bytes": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_uint64)]),
    "vv_cfg_norm_coef": (C.c_int, [C.c_void_p, C.POINTER(vv_cfg_norm_coef_args), C.c_void_p]),
    "vv_ode_stage_norm": (C.c_int, [C.c_void_p, C.POINTER(vv_ode_stage_args), C.c_void_p, C.c_void_p, C.c_void_p]),
    "vv_transformer_steps_reuse": (C.c_int, [C.c_void_p, C.POINTER(vv_steps_args), C.c_void_p, C.c_int, C.POINTER(vv_reuse_args), C.c_void_p]),
    "vv_transformer_reuse_ws_bytes": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_uint64)]),
    "vv_ode_stage_reuse": (C.c_int, [C.c_void_p, C.POINTER(vv_ode_stage_args), C.c_void_p, C.POINTER(vv_reuse_stage_args), C.c_void_p]),
    "vv_cfg_drift_reduce": (C.c_int, [C.c_void_p, C.POINTER(vv_cfg_drift_args), C.c_void_p]),
    "vv_transformer_steps_cached": (C.c_int, [C.c_void_p, C.POINTER(vv_steps_args), C.POINTER(vv_block_cache_args), C.c_void_p]),
    "vv_transformer_cached_ws_bytes": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_uint64)]),
    "vv_block_span": (C.c_int, [C.c_void_p, C.POINTER(vv_block_span_args), C.c_void_p]),
    "vv_block_drift_reduce": (C.c_int, [C.c_void_p, C.POINTER(vv_block_drift_args), C.c_void_p]),
    "vv_preprocess": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vv_preprocess_h": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vv_transformer_steps": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "vv_transformer_steps_h": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "vv_transformer_ws_bytes": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_uint64)]),
    "vv_transformer_steps_into": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p]),
    "vv_decode": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                            C.c_void_p, C.c_void_p, C.c_void_p]),
    "vv_decode_ws_bytes": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_uint64)]),
    "vv_decode_into": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    "vv_ws_generation": (C.c_uint64, [C.c_void_p]),
    "vv_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    "vv_set_rope_theta": (C.c_int, [C.c_void_p, C.c_float]),
    "vv_prof_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "vv_prof_collect": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vv_gemm": (C.c_int, [C.c_void_p, C.POINTER(vv_gemm_args), C.c_void_p]),
    "vv_attention": (C.c_int, [C.c_void_p, C.POINTER(vv_attn_args), C.c_void_p]),
    "vv_layernorm": (C.c_int, [C.c_void_p, C.POINTER(vv_ln_args), C.c_void_p]),
    "vv_posconv": (C.c_int, [C.c_void_p, C.POINTER(vv_posconv_args), C.c_void_p]),
    "vv_conv1d": (C.c_int, [C.c_void_p, C.POINTER(vv_conv_args), C.c_void_p]),
    "vv_mrf_resblock": (C.c_int, [C.c_void_p, C.POINTER(vv_mrf_args), C.c_void_p]),
    "vv_conv_post": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int,
                               C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p]),
    "vv_mel": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "vv_groupnorm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                               C.c_int, C.c_void_p]),
    "vv_text_embed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                C.c_void_p]),
    "vv_dwconv": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                            C.c_void_p]),
    "vv_grn": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                         C.c_void_p]),
    "vv_rope_compact": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "vv_conv_split_bytes": (C.c_uint64, [C.c_int32, C.c_int32, C.c_int32]),
    "vv_conv_split_weights": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "vv_gemm_tail_plan": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "vv_rope_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "vv_cfg_euler": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p]),
    "vv_cfg_euler_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p]),
    "vv_pack_cat": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                              C.c_void_p, C.c_void_p]),
    "vv_pack_cat_guided": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vv_row_tables": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vv_guided_tables": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vv_ref_len": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "vv_decode_len": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "vv_vocos_lens": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "vv_mel_slice": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "vv_vocos_im2col_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                     C.c_void_p]),
    "vv_vocos_spectrum": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "vv_vocos_ola": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int,
                               C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "vv_resample_poly": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "vv_ingest_pcm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p]),
    "vv_normalize_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int64]),
    "vv_normalize_clips": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vv_edit_splice": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "vv_preprocess_edit": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "vv_noise_fill": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "vv_edit_restore": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "vv_join_chunks": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                 C.c_int64, C.c_int, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "vv_pcm_resample": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                  C.c_int, C.c_void_p, C.c_int64, C.c_void_p]),
    "vv_pcm_encode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]),
    "vv_pcm_loudness_ws_bytes": (C.c_uint64, [C.c_int64, C.c_int]),
    "vv_pcm_loudness": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_int64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    "vv_pcm_limit_tile": (C.c_int, [C.c_int]),
    "vv_pcm_limit_ws_bytes": (C.c_uint64, [C.c_int64, C.c_int64, C.c_int]),
    "vv_pcm_limit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    "vv_flac_frame_bound": (C.c_uint64, [C.c_int64]),
    "vv_pcm_flac_ws_bytes": (C.c_uint64, [C.c_int64, C.c_int]),
    "vv_pcm_flac_lpc_ws_bytes": (C.c_uint64, [C.c_int64, C.c_int, C.c_int]),
    "vv_pcm_flac_lpc": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64,
                                  C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    "vv_pcm_flac": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p,
                              C.c_void_p, C.c_uint64, C.c_void_p]),
    "vv_flac_decode_frame_bound": (C.c_uint64, [C.c_int, C.c_int, C.c_int]),
    "vv_flac_index_ws_bytes": (C.c_uint64, [C.c_int64, C.c_int]),
    "vv_flac_decode_ws_bytes": (C.c_uint64, [C.c_int64, C.c_int64]),
    "vv_flac_index": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    "vv_flac_decode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                 C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    "vv_pcm_adpcm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]),
    "vv_wav_decode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "vv_pcm_stretch_ws_bytes": (C.c_uint64, [C.c_int]),
    "vv_pcm_stretch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                 C.c_int64, C.c_void_p, C.c_uint64, C.c_void_p]),
    "vv_pcm_formant_ws_bytes": (C.c_uint64, [C.c_int64, C.c_int]),
    "vv_pcm_formant": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_uint64, C.c_void_p]),
    "vv_pcm_denoise_ws_bytes": (C.c_uint64, [C.c_int]),
    "vv_pcm_denoise": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_uint64, C.c_void_p]),
    "vv_pcm_denoise_bias_ws_bytes": (C.c_uint64, [C.c_int64, C.c_int]),
    "vv_pcm_denoise_bias": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_int64, C.c_void_p, C.c_uint64, C.c_void_p]),
    "vv_pcm_watermark_ws_bytes": (C.c_uint64, [C.c_int]),
    "vv_pcm_watermark": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_double, C.c_double,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_uint64, C.c_void_p]),
    "vv_pcm_watermark_detect_ws_bytes": (C.c_uint64, [C.c_int64, C.c_int]),
    "vv_pcm_watermark_detect": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_uint64, C.c_void_p]),
    "vv_set_vocos": (C.c_int, [C.c_void_p, C.POINTER(vv_vocos_cfg)]),
    "vv_vocos_im2col": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "vv_istft_head": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                C.c_void_p]),
}

_lib = None
_lib_lock = threading.Lock()


def load_library(path: Optional[str] = None):
    """dlopen the in-tree library and type every export of include/vvtts.h.  No compute happens."""
    global _lib
    with _lib_lock:
        if _lib is not None and path is None:
            return _lib
        p = path or LIB_PATH
        if not os.path.exists(p):
            raise HipUnavailable(f"{p} not found: build it with `python __graft_entry__.py` (hipcc --offload-arch=gfx950); "
                                 "the HIP synthesis path has no CPU fallback")
        lib = C.CDLL(p)
        for name, (res, args) in EXPORTS.items():
            fn = getattr(lib, name)          # AttributeError if an export is missing
            fn.restype, fn.argtypes = res, args
        if path is None:
            _lib = lib
        return lib


def cfg_from_spec(spec: ModelSpec) -> vv_model_cfg:
    c = vv_model_cfg()
    c.n_mel, c.n_fft, c.win_length, c.hop_length = spec.n_mel, spec.n_fft, spec.win_length, spec.hop_length
    c.dim, c.depth, c.heads, c.head_dim, c.ff_mult = spec.dim, spec.depth, spec.heads, spec.head_dim, spec.ff_mult
    c.text_dim, c.text_layers, c.text_conv_k, c.text_ff_mult = spec.text_dim, spec.text_layers, spec.text_conv_k, spec.text_ff_mult
    c.vocab_rows = spec.vocab_size + 1
    c.pos_conv_k, c.pos_conv_groups, c.time_freq_dim = spec.pos_conv_k, spec.pos_conv_groups, spec.time_freq_dim
    c.cfg_strength = spec.cfg_strength
    c.voc_pre_ch, c.voc_pre_k, c.voc_post_k = spec.voc_pre_ch, spec.voc_pre_k, spec.voc_post_k
    c.voc_n_up = len(spec.voc_up_rates)
    for i, (r, k) in enumerate(zip(spec.voc_up_rates, spec.voc_up_kernels)):
        c.voc_up_rates[i], c.voc_up_kernels[i] = r, k
    c.voc_n_res = len(spec.voc_res_kernels)
    for i, k in enumerate(spec.voc_res_kernels):
        c.voc_res_kernels[i] = k
    c.voc_n_dil = len(spec.voc_res_dilations)
    for i, d in enumerate(spec.voc_res_dilations):
        c.voc_res_dilations[i] = d
    c.voc_lrelu = spec.voc_lrelu
    c.max_pos = pack.MAX_POS
    return c


def vocos_cfg_from_spec(spec: ModelSpec) -> vv_vocos_cfg:
    v = vv_vocos_cfg()
    v.dim, v.intermediate, v.layers = spec.vocos_dim, spec.vocos_intermediate, spec.vocos_layers
    v.embed_k, v.dw_k, v.ln_eps = spec.vocos_embed_k, spec.vocos_dw_k, spec.vocos_ln_eps
    v.n_fft, v.win_length, v.hop_length = spec.n_fft, spec.win_length, spec.hop_length
    return v


def _dt(s) -> Tuple[int, torch.dtype]:
    if s in ("bf16", "bfloat16", torch.bfloat16, VV_BF16):
        return VV_BF16, torch.bfloat16
    if s in ("fp32", "f32", "float32", torch.float32, VV_F32):
        return VV_F32, torch.float32
    raise ValueError(f"acoustic dtype must be bf16 or fp32, got {s!r}")


def _host_lens(B: int, values):
    """B per-item lengths on the host, as the int32 array the ``*_h`` entries and ``seq_len_host`` fields take."""
    return (C.c_int32 * B)(*[int(v) for v in values])


def _pre_ptrs(pre) -> Tuple[int, ...]:
    """The conditioning and rope tables of a ``pre`` dict as pointers, in the order the step entries take them."""
    return tuple(pre[k].data_ptr() for k in ("cat_mel_text", "cat_mel_text_drop", "rope_cos_q", "rope_sin_q", "rope_cos_k", "rope_sin_k"))


class HipSynth(PcmStage):
    """One GPU's synthesis engine: weights resident in HBM, three device-resident stages, and the PCM stage of pcm_stage.py.

    flat_weights: optional pre-filled flat uint8 device buffer (e.g. received by RCCL broadcast);
    otherwise ``weights`` (fp32 CPU dict) is packed and uploaded here.
    """

    def __init__(self, spec: ModelSpec, weights: Optional[Dict[str, torch.Tensor]] = None, device: str = "cuda:0",
                 acoustic_dtype="bf16", nfe_step: int = 32, flat_weights: Optional[torch.Tensor] = None, ode_method="euler",
                 ode_report: bool = False, cfg_zero_init: int = 0):
        super().__init__()
        self.lib = load_library()
        if not torch.cuda.is_available():
            raise HipUnavailable("no HIP device is visible to torch; the synthesis hot path runs only on the GPU")
        self.spec = spec
        self.device = torch.device(device)
        self.dt_code, self.dt_torch = _dt(acoustic_dtype)
        self._lock = threading.RLock()       # one stream of calls per context (reference: api/tts_engine.py:64-67); re-entrant: reading_rope_tables
        self.ctx = C.c_void_p()
        cfg = cfg_from_spec(spec)
        idx = self.device.index if self.device.index is not None else 0
        rc = self.lib.vv_create(C.byref(self.ctx), idx, C.byref(cfg), self.dt_code)
        if rc != 0:
            raise HipUnavailable(f"vv_create failed ({rc}): {self.lib.vv_last_error(None).decode()}")
        if spec.vocoder == "vocos":                  # N6: before any weight is bound (vv_finalize_weights then checks the Vocos names)
            self._check(self.lib.vv_set_vocos(self.ctx, C.byref(vocos_cfg_from_spec(spec))))
        table, total = pack.plan(spec, self.dt_torch)
        if flat_weights is None:
            if weights is None:
                raise ValueError("either weights or flat_weights is required")
            cpu = torch.zeros(total, dtype=torch.uint8)
            pack.fill(spec, self.dt_torch, weights, cpu)
            flat_weights = cpu.to(self.device)
        assert flat_weights.dtype == torch.uint8 and flat_weights.numel() >= total and flat_weights.is_cuda
        self.flat = flat_weights
        base = self.flat.data_ptr()
        for name, off, nb in table:
            self._check(self.lib.vv_bind_weight(self.ctx, name.encode(), base + off, nb))
        self._check(self.lib.vv_finalize_weights(self.ctx))
        cq, sq, ck, sk = pack.rope_tables(spec)
        self.rope = tuple(t.to(self.device) for t in (cq, sq, ck, sk))
        self._vocoder_bias = None        # N19: the decoder's bias profile, float64 [1][513] on the device (vocoder_bias)
        # the tables this engine hands to the transformer stage are the standard ones of spec.rope_theta: the bf16 model may compute the
        # angles in the QKV epilogue instead of reading them (vv_set_rope_theta; the fp32 model reads the tables either way)
        self.grid_generation = 0         # bumped by whatever a captured Euler-step graph has baked in (time grid, rope mode, options)
        self.set_rope_theta(float(spec.rope_theta))
        self.nfe_step = None
        self.ode_method = None           # the solver of the plan in force: a name of model_spec.ODE_METHODS / ODE_MULTISTEP or a custom tableau (a, b)
        self.ode_report = False          # N20: every transformer_steps call from step 0 leaves its step report (last_ode_report); needs a multistep plan
        self._ode_report = None          # the last call's report, float64 [n_steps, B, 2] on the device
        self.cfg_reuse_report = False    # N21: every transformer_steps call with a mask leaves its drift report (last_cfg_reuse_report)
        self._cfg_reuse_report = None    # the last such call's report, float64 [n_evals, B, 2] on the device
        self.block_cache_report = False  # N23: every transformer_steps call with a block cache leaves its report (last_block_cache_report)
        self._block_cache_report = None  # the last such call's report, float64 [n_evals, B, 2, 2] on the device
        self.cfg_norm_report = False     # N24: every transformer_steps call with CFG-Zero* / rescale leaves its (s, f) (last_cfg_norm_report)
        self._cfg_norm_report = None     # the last such call's report, fp32 [n_evals, B, 2] on the device
        self.cfg_zero_init = None        # N24 zero-init: the leading steps the plan in force leaves out
        self.set_nfe(nfe_step, ode_method, cfg_zero_init)
        self.set_ode_report(ode_report)

    # ------------------------------------------------------------------ plumbing
    def _check(self, rc: int):
        if rc != 0:
            raise RuntimeError(f"vvtts HIP call failed ({rc}): {self.lib.vv_last_error(self.ctx).decode()}")

    def _stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream

    def close(self):
        if getattr(self, "ctx", None) is not None and self.ctx.value:
            self.lib.vv_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_nfe(self, nfe_step: int, ode_method="euler", cfg_zero_init: int = 0):
        """The sampler's plan (N7): ``nfe_step`` grid points = ``nfe_step - 1`` ODE steps of the explicit Runge-Kutta method
        ``ode_method`` (a name of model_spec.ODE_METHODS, or a tableau (a, b)); ``n_evals`` = stages x steps DiT evaluations.  Or (N20) a
        name of model_spec.ODE_MULTISTEP: Adams-Bashforth on the slopes kept from the steps before, one evaluation per step
        (vv_set_ode_multistep); a transformer_steps call then starts at step 0.  ``cfg_zero_init`` = K (N24): the plan of the grid's steps
        K ... nfe_step - 2 alone (model_spec.ode_plan(skip=K)); steps, evaluations, masks and reports are then those of that plan."""
        if not isinstance(ode_method, str):
            ode_method = (tuple(tuple(r) for r in ode_method[0]), tuple(ode_method[1]))
        if (nfe_step, ode_method, cfg_zero_init) == (self.nfe_step, self.ode_method, self.cfg_zero_init):
            return
        if nfe_step < 2:
            raise ValueError("nfe_step must be >= 2")
        if self.ode_report and not (isinstance(ode_method, str) and ode_method in ODE_MULTISTEP):
            raise ValueError("ode_report is on: it needs a multistep ode_method (set_ode_report(False) first)")
        plan = ode_plan(nfe_step, self.spec.sway_coef, ode_method, cfg_zero_init)
        n_steps = int(plan.dt.numel())
        if n_steps * plan.s > ODE_MAX_EVALS:
            raise ValueError(f"{n_steps} ODE steps of {plan.s} stages exceed {ODE_MAX_EVALS} evaluations")
        sinus = pack.time_sinus_table(self.spec, plan.t).contiguous()
        dtc = plan.dt.contiguous()
        a = (C.c_double * (plan.s * plan.s))(*[v for r in plan.a for v in r])
        b = (C.c_double * plan.s)(*plan.b)
        with self._lock, torch.cuda.device(self.device):          # under the engine lock: no step call or graph replay runs across the change
            if plan.beta is not None:                             # N20: the Euler tables and the weights of the kept slopes
                q = len(plan.beta[0])
                beta = (C.c_double * (n_steps * q))(*[v for r in plan.beta for v in r])
                self._check(self.lib.vv_set_ode_multistep(self.ctx, sinus.data_ptr(), dtc.data_ptr(), n_steps, q, beta, self._stream()))
            else:
                self._check(self.lib.vv_set_ode_plan(self.ctx, sinus.data_ptr(), dtc.data_ptr(), n_steps, plan.s, a, b, self._stream()))
            self.nfe_step = nfe_step
            self.ode_method = ode_method
            self.cfg_zero_init = int(cfg_zero_init)
            self.n_steps = n_steps
            self.n_evals = n_steps * plan.s
            self.plan = plan             # the evaluation times a guidance interval is compared with (guidance_mask)
            self._t_host = (C.c_float * self.n_evals)(*[float(v) for v in plan.t])     # the same times for projected guidance (vv_apg_args.t_host)
            self.grid_generation += 1    # vv_set_ode_plan frees and reallocates the tables a captured step graph points into

    def set_ode_report(self, on: bool):
        """N20: turn the step report of the multistep plan in force on or off (ModelConfig.ode_report).  On, every transformer_steps call
        that starts at step 0 leaves float64 [n_steps, B, 2] for last_ode_report; off (the default) launches and allocates nothing."""
        on = bool(on)
        if on and self.plan.beta is None:
            raise ValueError(f"ode_report needs a multistep ode_method ({sorted(ODE_MULTISTEP)}), the plan in force is {self.ode_method!r}")
        with self._lock:
            self.ode_report = on
            if not on:
                self._ode_report = None

    def last_ode_report(self):
        """N20: the step report of the last transformer_steps call, numpy float64 [n_steps, B, 2]: per step n and item b (D2, F2) =
        (sum (f_n - f_{n-1})^2, sum f_n^2) over the item's frames and the n_mel columns, f_n the combined velocity of step n (after
        guidance and the projected term); row 0 holds (0, F2).  sqrt(D2 / F2) is the relative change of the velocity over the step,
        the local-error term of an Euler step.  One copy from the device; None when no call has left a report."""
        with self._lock:
            rep = self._ode_report
        return None if rep is None else rep.cpu().numpy()

    def set_cfg_reuse_report(self, on: bool):
        """N21: turn the drift report of guidance reuse on or off (ModelConfig.cfg_reuse_report).  On, every transformer_steps call with a
        guidance mask leaves float64 [n_evals, B, 2] for last_cfg_reuse_report (two small launches per evaluation and lane); off (the
        default) launches and allocates nothing."""
        with self._lock:
            self.cfg_reuse_report = bool(on)
            if not on:
                self._cfg_reuse_report = None

    def last_cfg_reuse_report(self):
        """N21: the drift report of the last transformer_steps call that had a mask, numpy float64 [n_evals, B, 2]: per evaluation e and
        item b (E2, N2) = (sum (D_e - D_stored)^2, sum D_e^2) over the item's frames and the n_mel columns where b's unconditional
        prediction is computed at e, D = p_c - p_u and D_stored the difference of b's previous computed evaluation of the call (E2 = 0
        at the first); (0, 0) where b reuses or is not guided, and at evaluations outside the call.  sqrt(E2 / N2) is how far the
        difference moved over the evaluations it was reused for.  One copy from the device; None when no call has left a report."""
        with self._lock:
            rep = self._cfg_reuse_report
        return None if rep is None else rep.cpu().numpy()

    def set_block_cache_report(self, on: bool):
        """N23: turn the report of block caching on or off (ModelConfig.block_cache_report).  On, every transformer_steps call with a
        block cache stores at each full evaluation and leaves float64 [n_evals, B, 2, 2] for last_block_cache_report; off (the default)
        launches and allocates nothing for it."""
        with self._lock:
            self.block_cache_report = bool(on)
            if not on:
                self._block_cache_report = None

    def last_block_cache_report(self):
        """N23: the report of the last transformer_steps call that cached blocks, numpy float64 [n_evals, B, 2, 2]: per evaluation e, item
        b and CFG branch (0 conditional, 1 unconditional) (E2, N2) = (sum (C_e - C_stored)^2, sum C_e^2) over the item's frames and the
        model's columns, C the contribution of the span of blocks to the residual stream at a full evaluation and C_stored the one of
        the previous full evaluation of the call (E2 = 0 at the first); (0, 0) at a light evaluation and outside the call.
        sqrt(E2 / N2) is how far the contribution moved between two full evaluations.  One copy from the device; None when no call has
        left a report."""
        with self._lock:
            rep = self._block_cache_report
        return None if rep is None else rep.cpu().numpy()

    def block_cache_modes(self, block_cache, interval=None) -> Optional[torch.Tensor]:
        """N23: the ``block_modes`` of transformer_steps_ex for ``block_cache`` = (first, last, every) on the plan in force
        (model_spec.block_cache_schedule, with this engine's report switch) -> (first, last, uint8 host tensor [n_evals]); None for None."""
        bc = check_block_cache(block_cache, self.spec.depth)
        if bc is None:
            return None
        return bc[0], bc[1], block_cache_schedule(self.plan, bc[2], interval, self.block_cache_report)

    def cached_ws_bytes(self, B: int, N: int, seq_len_host, report: bool = False) -> int:
        """Bytes of a caller-owned workspace for a call that caches blocks (vv_transformer_cached_ws_bytes; the same for every schedule):
        the plain figure plus one fp32 plane of the lane's rows x the model's width per lane, plus a second plane and the partial sums
        when ``report``."""
        nb = C.c_uint64()
        with self._lock, self._SizedAsTheCall(self, B):
            self._check(self.lib.vv_transformer_cached_ws_bytes(self.ctx, int(B), int(N), _host_lens(B, seq_len_host), int(bool(report)), C.byref(nb)))
        return int(nb.value)

    class _ReportScope:
        """The report buffer of one steps call: set in front of it, cleared behind it whatever happens (the library keeps no pointer to a
        tensor that may be freed)."""
        def __init__(self, eng, B, step0):
            self.eng, self.buf = eng, None
            if eng.ode_report and step0 == 0:
                self.buf = torch.zeros((eng.n_steps, int(B), 2), dtype=torch.float64, device=eng.device)

        def __enter__(self):
            if self.buf is not None:
                self.eng._check(self.eng.lib.vv_set_ode_report(self.eng.ctx, self.buf.data_ptr(), self.eng.n_steps, int(self.buf.shape[1])))
            return self

        def __exit__(self, et, ev, tb):
            if self.buf is not None:
                self.eng.lib.vv_set_ode_report(self.eng.ctx, None, 0, 0)
                self.eng._ode_report = self.buf if et is None else None
            return False

    # ------------------------------------------------------------------ stages
    def preprocess(self, audio: torch.Tensor, audio_len: torch.Tensor, text_ids: torch.Tensor, text_len: torch.Tensor,
                   seq_len: torch.Tensor, N: int, max_audio_len: Optional[int] = None, seq_len_host=None,
                   audio_len_host=None) -> Dict[str, torch.Tensor]:
        """audio int16 [B,S], text_ids int32 [B,T], *_len int32 [B] -- all on the device.  audio_len_host (optional, the same
        values as audio_len): lets the call refuse a clip too short for the centred STFT (< n_fft/2 + 1 samples) before launching."""
        B = audio.shape[0]
        for t, d in ((audio, torch.int16), (audio_len, torch.int32), (text_ids, torch.int32), (text_len, torch.int32), (seq_len, torch.int32)):
            assert t.is_cuda and t.dtype == d and t.is_contiguous(), "preprocess inputs must be contiguous device tensors"
        s = self.spec
        cat = torch.empty((B, N, s.cond_dim), dtype=torch.float32, device=self.device)
        cat_drop = torch.empty_like(cat)
        ref_len = torch.empty((B,), dtype=torch.int32, device=self.device)
        mal = int(max_audio_len if max_audio_len is not None else audio.shape[1])
        with self._lock, torch.cuda.device(self.device):
            if audio_len_host is not None:
                self._check(self.lib.vv_preprocess_h(self.ctx, B, N, audio.data_ptr(), audio.shape[1], mal, audio_len.data_ptr(), _host_lens(B, audio_len_host),
                                                     text_ids.data_ptr(), text_ids.shape[1], text_len.data_ptr(), seq_len.data_ptr(),
                                                     cat.data_ptr(), cat_drop.data_ptr(), ref_len.data_ptr(), self._stream()))
            else:
                self._check(self.lib.vv_preprocess(self.ctx, B, N, audio.data_ptr(), audio.shape[1], mal, audio_len.data_ptr(),
                                                   text_ids.data_ptr(), text_ids.shape[1], text_len.data_ptr(), seq_len.data_ptr(),
                                                   cat.data_ptr(), cat_drop.data_ptr(), ref_len.data_ptr(), self._stream()))
        return self._pre_dict(cat, cat_drop, ref_len, seq_len, N, seq_len_host)

    def _pre_dict(self, cat, cat_drop, ref_len, seq_len, N, seq_len_host):
        return {"cat_mel_text": cat, "cat_mel_text_drop": cat_drop, "ref_signal_len": ref_len, "seq_len": seq_len,
                "seq_len_host": None if seq_len_host is None else [int(v) for v in seq_len_host],
                "rope_cos_q": self.rope[0][:N], "rope_sin_q": self.rope[1][:N], "rope_cos_k": self.rope[2][:N],
                "rope_sin_k": self.rope[3][:N]}

    def max_rows_per_call(self) -> int:
        """Upper bound on sum(seq_len) of one transformer_steps call: the packed qkv buffer (2 branches x rows x 3D) must stay
        below 2 GiB (32-bit byte offsets in the kernels)."""
        es = 2 if self.dt_torch == torch.bfloat16 else 4
        return ((1 << 31) - 1) // (2 * 3 * self.spec.dim * es)

    def guidance_mask(self, interval, strengths, reuse=None) -> Optional[torch.Tensor]:
        """model_spec.guidance_mask on the plan in force: the ``guide`` of transformer_steps for a guidance interval (one for every item
        or one per item) and the B strengths (a None strength = the model's); None = every item guided everywhere.  reuse (N21): None,
        one k or one per item -- the unconditional branch at every k-th guided evaluation of an item, a 2 in the mask in between."""
        return guidance_mask(self.plan, interval, [self.spec.cfg_strength if v is None else v for v in strengths], reuse)

    def apg_tensors(self, etas, norms):
        """N11: the ``apg`` of transformer_steps from B host values each -- eta (None = 1) and the RMS cap (None = no cap), validated by
        model_spec.check_apg.  None when projected guidance is off for every item (the call then goes to the existing entries), else
        (eta, norm) fp32 [B] on the device, a cap of 0 standing for "none"."""
        etas, norms = list(etas), list(norms)
        if len(etas) != len(norms):
            raise ValueError("apg_tensors: one eta and one norm per item")
        pairs = [check_apg(e, r) for e, r in zip(etas, norms)]
        if all(p is None for p in pairs):
            return None
        eta = torch.tensor([1.0 if p is None else p[0] for p in pairs], dtype=torch.float32).to(self.device)
        norm = torch.tensor([0.0 if p is None or p[1] is None else p[1] for p in pairs], dtype=torch.float32).to(self.device)
        return eta, norm

    def cfg_norm_tensors(self, stars, rescales):
        """N24: the ``cfg_norm`` of transformer_steps from B host values each -- the CFG-Zero* switch (None / False = off) and the rescale phi
        (None = off), validated by model_spec.check_cfg_norm.  None when both are off for every item (the call then goes to the existing
        entries), else (star, rescale) fp32 [B] on the device, 0 standing for "off"."""
        stars, rescales = list(stars), list(rescales)
        if len(stars) != len(rescales):
            raise ValueError("cfg_norm_tensors: one cfg_zero_star and one cfg_rescale per item")
        pairs = [check_cfg_norm(z, r) for z, r in zip(stars, rescales)]
        if all(p is None for p in pairs):
            return None
        star = torch.tensor([0.0 if p is None or not p[0] else 1.0 for p in pairs], dtype=torch.float32).to(self.device)
        resc = torch.tensor([0.0 if p is None else p[1] for p in pairs], dtype=torch.float32).to(self.device)
        return star, resc

    def set_cfg_norm_report(self, on: bool):
        """N24: on, every transformer_steps call with cfg_norm leaves fp32 [n_evals, B, 2] for last_cfg_norm_report (the coefficient kernel
        writes its pair twice: no further launch); off (the default) allocates nothing."""
        with self._lock:
            self.cfg_norm_report = bool(on)
            if not on:
                self._cfg_norm_report = None

    def last_cfg_norm_report(self):
        """N24: the (s, f) of the last transformer_steps call with cfg_norm, numpy float32 [n_evals, B, 2]: per evaluation e of the plan in
        force and item b the optimised scale and the rescale factor the stage kernel used, (1, 1) where b is not guided, and zeros at
        evaluations outside the call.  One copy from the device; None when no call has left a report."""
        with self._lock:
            rep = self._cfg_norm_report
            return None if rep is None else rep.cpu().numpy()

    def norm_ws_bytes(self, B: int, N: int, seq_len_host) -> int:
        """Bytes of a caller-owned workspace for a call with CFG-Zero* / rescale (vv_transformer_norm_ws_bytes; the same with any mask)."""
        return self._steps_ws_bytes(self.lib.vv_transformer_norm_ws_bytes, B, N, _host_lens(B, seq_len_host))

    def transformer_steps(self, x: torch.Tensor, pre: Dict[str, torch.Tensor], step0: int, n_steps: int, seq_len_host=None,
                          cfg: Optional[torch.Tensor] = None, guide: Optional[torch.Tensor] = None, apg=None, block_cache=None,
                          block_cache_interval=None, cfg_norm=None) -> torch.Tensor:
        """x fp32 [B,N,n_mel] updated in place on the device.  seq_len_host (optional list / array of the B lengths, the same
        values as pre["seq_len"]): the call then needs no read-back and no stream synchronisation (vv_transformer_steps_h).
        cfg (optional fp32 [B] on the device): the guidance strength of each item (vv_transformer_steps_ex); None = the model's.
        guide (optional uint8 [n_evals, B] on the HOST, N8): guided(b, e) of every evaluation of the plan in force
        (vv_transformer_steps_guided; model_spec.guidance_mask builds it); None = every item guided everywhere.  A mask that holds a 2
        (N21 guidance reuse), or any mask while the drift report is on, goes to vv_transformer_steps_reuse.
        apg (optional pair (eta, norm) of fp32 [B] device tensors, either None, N11): projected guidance per item
        (vv_transformer_steps_apg; apg_tensors builds it); None, or a pair of Nones = off: the existing entries.
        block_cache (optional (first, last, every), N23): the blocks [first, last) are skipped at every evaluation inside
        block_cache_interval (None = everywhere) whose count is not a multiple of ``every`` (vv_transformer_steps_cached;
        model_spec.block_cache_schedule builds the modes); never with a mask or apg.  None = the existing entries.
        cfg_norm (optional pair (star, rescale) of fp32 [B] device tensors, either None, N24): CFG-Zero*'s optimised scale and the guidance
        rescale per item (vv_transformer_steps_norm; cfg_norm_tensors builds it); never with apg, block_cache or a mask that holds a 2."""
        B, N, M = x.shape
        assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and M == self.spec.n_mel
        if seq_len_host is None:
            seq_len_host = pre.get("seq_len_host")
        if apg is not None and apg[0] is None and apg[1] is None:
            apg = None
        if cfg_norm is not None and cfg_norm[0] is None and cfg_norm[1] is None:
            cfg_norm = None
        modes = self.block_cache_modes(block_cache, block_cache_interval)
        if cfg is not None or guide is not None or apg is not None or modes is not None or cfg_norm is not None:
            assert cfg is None or (cfg.is_cuda and cfg.dtype == torch.float32 and cfg.is_contiguous() and cfg.shape == (B,)), "cfg: fp32 [B] on the device"
            host = None if seq_len_host is None else _host_lens(B, seq_len_host)
            self.transformer_steps_ex(x, pre, step0, n_steps, host, cfg, guide=guide, apg=apg, block_modes=modes, cfg_norm=cfg_norm)
            return x
        with self._lock, torch.cuda.device(self.device), self._ReportScope(self, B, step0):
            tail = _pre_ptrs(pre) + (step0, n_steps, self._stream())
            if seq_len_host is not None:
                self._check(self.lib.vv_transformer_steps_h(self.ctx, B, N, pre["seq_len"].data_ptr(), _host_lens(B, seq_len_host), x.data_ptr(), *tail))
            else:
                self._check(self.lib.vv_transformer_steps(self.ctx, B, N, pre["seq_len"].data_ptr(), x.data_ptr(), *tail))
        return x

    class _SizedAsTheCall:
        """A size query sees the context as the next steps call will: under the step report (N20) the library keeps one more slope and the
        report's partial sums, and it knows of the report only while a buffer is set (_ReportScope sets one around every call).  Without
        this the bytes a query names were too few for a call under set_ode_report(True)."""
        def __init__(self, eng, B):
            self.eng, self.buf = eng, None
            if eng.ode_report:
                self.buf = torch.zeros((eng.n_steps, int(B), 2), dtype=torch.float64, device=eng.device)

        def __enter__(self):
            if self.buf is not None:
                self.eng._check(self.eng.lib.vv_set_ode_report(self.eng.ctx, self.buf.data_ptr(), self.eng.n_steps, int(self.buf.shape[1])))
            return self

        def __exit__(self, et, ev, tb):
            if self.buf is not None:
                self.eng.lib.vv_set_ode_report(self.eng.ctx, None, 0, 0)
            return False

    def _steps_ws_bytes(self, entry, B: int, N: int, host) -> int:
        """One of the three size queries of the transformer stage (``entry``) for the B host lengths ``host`` (a ctypes int32 array)."""
        nb = C.c_uint64()
        with self._lock, self._SizedAsTheCall(self, B):
            self._check(entry(self.ctx, int(B), int(N), host, C.byref(nb)))
        return int(nb.value)

    def guided_ws_bytes(self, B: int, N: int, seq_len_host) -> int:
        """Bytes of a caller-owned workspace for a call with a guidance mask (vv_transformer_guided_ws_bytes; the same for every mask)."""
        return self._steps_ws_bytes(self.lib.vv_transformer_guided_ws_bytes, B, N, _host_lens(B, seq_len_host))

    def reuse_ws_bytes(self, B: int, N: int, seq_len_host, report: bool = False) -> int:
        """Bytes of a caller-owned workspace for a call that reuses guidance differences (vv_transformer_reuse_ws_bytes; the same for every
        mask): the guided figure plus one difference buffer per lane, plus the drift report's partial sums when ``report``."""
        nb = C.c_uint64()
        with self._lock, self._SizedAsTheCall(self, B):
            self._check(self.lib.vv_transformer_reuse_ws_bytes(self.ctx, int(B), int(N), _host_lens(B, seq_len_host), int(bool(report)), C.byref(nb)))
        return int(nb.value)

    def apg_ws_bytes(self, B: int, N: int, seq_len_host) -> int:
        """Bytes of a caller-owned workspace for a call with projected guidance (vv_transformer_apg_ws_bytes; the same with any mask)."""
        return self._steps_ws_bytes(self.lib.vv_transformer_apg_ws_bytes, B, N, _host_lens(B, seq_len_host))

    def transformer_steps_ex(self, x: torch.Tensor, pre: Dict[str, torch.Tensor], step0: int, n_steps: int, host=None,
                             cfg: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None,
                             guide: Optional[torch.Tensor] = None, apg=None, reuse_entry: Optional[bool] = None, block_modes=None,
                             cfg_norm=None) -> None:
        """The struct-argument entry as it is (vv_transformer_steps_ex); raises on a non-zero code.  host: a ctypes int32 array of
        the B lengths or None (read back); ws: an optional caller-owned uint8 workspace (needs host).  guide: a contiguous uint8
        HOST tensor [n_evals of the plan in force, ld_guide], handed to vv_transformer_steps_guided as it is (the library checks
        ld_guide >= B).  apg: None, or a pair (eta, norm) of fp32 [B] device tensors (either None), handed to
        vv_transformer_steps_apg with the times of the plan in force.  reuse_entry (N21): True hands the mask to
        vv_transformer_steps_reuse (with the drift report's buffer when set_cfg_reuse_report is on), False never; None = when the mask
        holds a 2 or the report is on.  Never together with apg.  block_modes (N23): None, or (first, last, modes) with modes a
        contiguous uint8 HOST tensor [n_modes], handed to vv_transformer_steps_cached as they are (with the report's buffer when
        set_block_cache_report is on); never together with guide or apg.  cfg_norm (N24): None, or a pair (star, rescale) of fp32 [B]
        device tensors (either None), handed to vv_transformer_steps_norm (with the report's buffer when set_cfg_norm_report is on); never
        together with apg, block_modes or a mask that holds a 2."""
        B, N, _ = x.shape
        if cfg_norm is not None:
            if len(cfg_norm) != 2 or any(t is not None and not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32
                                                                and t.is_contiguous() and t.shape == (B,)) for t in cfg_norm):
                raise ValueError("cfg_norm must be a pair (star, rescale) of fp32 [B] device tensors or Nones")
            if apg is not None:
                raise ValueError("CFG-Zero* / guidance rescale is not combined with projected guidance (apg): both rewrite the guided slope")
            if block_modes is not None:
                raise ValueError("CFG-Zero* / guidance rescale is not combined with block caching (that entry has no guided form)")
            if reuse_entry or (guide is not None and bool((guide[:, :B] == 2).any())):
                raise ValueError("CFG-Zero* / guidance rescale is not combined with guidance reuse (a reused item has no unconditional prediction to measure)")
            reuse_entry = False
        if block_modes is not None:
            if guide is not None or apg is not None:
                raise ValueError("block caching takes no guidance mask and no projected guidance (a guided subset moves the rows the cache stores)")
            first, last, modes = block_modes
            if not (isinstance(modes, torch.Tensor) and modes.device.type == "cpu" and modes.dtype == torch.uint8 and modes.dim() == 1 and modes.is_contiguous()):
                raise ValueError("block_modes is (first, last, a contiguous uint8 host tensor of one mode per evaluation)")
        if apg is not None:
            if len(apg) != 2 or any(t is not None and not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32
                                                           and t.is_contiguous() and t.shape == (B,)) for t in apg):
                raise ValueError("apg must be a pair (eta, norm) of fp32 [B] device tensors or Nones")
        if guide is not None:
            if not (isinstance(guide, torch.Tensor) and guide.device.type == "cpu" and guide.dtype == torch.uint8 and guide.dim() == 2
                    and guide.is_contiguous() and guide.shape[0] == self.n_evals):
                raise ValueError(f"guide must be a contiguous uint8 host tensor [{self.n_evals} evaluations, >= B]")
        a = vv_steps_args()
        a.B, a.N, a.seq_len, a.x = B, N, pre["seq_len"].data_ptr(), x.data_ptr()
        a.seq_len_host = None if host is None else C.cast(host, C.c_void_p)
        a.cat_mel_text, a.cat_mel_text_drop, a.rope_cos_q, a.rope_sin_q, a.rope_cos_k, a.rope_sin_k = _pre_ptrs(pre)
        a.step0, a.n_steps = int(step0), int(n_steps)
        if ws is not None:
            a.ws, a.ws_bytes = ws.data_ptr(), ws.numel()
        a.cfg_item = _ptr(cfg)
        if reuse_entry is None:
            reuse_entry = guide is not None and apg is None and (self.cfg_reuse_report or bool((guide[:, :B] == 2).any()))
        if reuse_entry and (apg is not None or guide is None):
            raise ValueError("guidance reuse needs a mask and is not combined with projected guidance (apg)")
        if apg is not None and guide is not None and bool((guide[:, :B] == 2).any()):
            raise ValueError("a mask that reuses guidance differences (a 2) is not combined with projected guidance (apg)")
        with self._lock, torch.cuda.device(self.device), self._ReportScope(self, B, step0):
            if block_modes is not None:
                rep = torch.zeros((self.n_evals, B, 2, 2), dtype=torch.float64, device=self.device) if self.block_cache_report else None
                k = vv_block_cache_args(int(first), int(last), modes.data_ptr(), int(modes.numel()), _ptr(rep), B, self.n_evals)
                self._block_cache_report = None
                self._check(self.lib.vv_transformer_steps_cached(self.ctx, C.byref(a), C.byref(k), self._stream()))
                self._block_cache_report = rep
            elif cfg_norm is not None:
                rep = torch.zeros((self.n_evals, B, 2), dtype=torch.float32, device=self.device) if self.cfg_norm_report else None
                q = vv_cfg_norm_args(_ptr(cfg_norm[0]), _ptr(cfg_norm[1]), _ptr(rep))
                self._cfg_norm_report = None
                self._check(self.lib.vv_transformer_steps_norm(self.ctx, C.byref(a), None if guide is None else guide.data_ptr(),
                                                               0 if guide is None else int(guide.shape[1]), C.byref(q), self._stream()))
                self._cfg_norm_report = rep
            elif reuse_entry:
                rep = torch.zeros((self.n_evals, B, 2), dtype=torch.float64, device=self.device) if self.cfg_reuse_report else None
                r = vv_reuse_args(_ptr(rep), B, self.n_evals)
                self._cfg_reuse_report = None
                self._check(self.lib.vv_transformer_steps_reuse(self.ctx, C.byref(a), guide.data_ptr(), int(guide.shape[1]), C.byref(r), self._stream()))
                self._cfg_reuse_report = rep
            elif apg is not None:
                q = vv_apg_args(_ptr(apg[0]), _ptr(apg[1]), C.cast(self._t_host, C.c_void_p))
                self._check(self.lib.vv_transformer_steps_apg(self.ctx, C.byref(a), None if guide is None else guide.data_ptr(),
                                                              0 if guide is None else int(guide.shape[1]), C.byref(q), self._stream()))
            elif guide is not None:
                self._check(self.lib.vv_transformer_steps_guided(self.ctx, C.byref(a), guide.data_ptr(), int(guide.shape[1]), self._stream()))
            else:
                self._check(self.lib.vv_transformer_steps_ex(self.ctx, C.byref(a), self._stream()))

    def decode(self, x: torch.Tensor, pre: Dict[str, torch.Tensor], t_gen_max: int, want_wave: bool = False):
        B, N, _ = x.shape
        hop = self.spec.hop_length
        pcm = torch.zeros((B, t_gen_max * hop), dtype=torch.int16, device=self.device)
        pcm_len = torch.empty((B,), dtype=torch.int32, device=self.device)
        wave = torch.zeros((B, t_gen_max * hop), dtype=torch.float32, device=self.device) if want_wave else None
        with self._lock, torch.cuda.device(self.device):
            self._check(self.lib.vv_decode(self.ctx, B, N, x.data_ptr(), pre["ref_signal_len"].data_ptr(), pre["seq_len"].data_ptr(),
                                           t_gen_max, pcm.data_ptr(), pcm.shape[1], pcm_len.data_ptr(), _ptr(wave), self._stream()))
        return (pcm, pcm_len, wave) if want_wave else (pcm, pcm_len)

    VOCODER_BIAS_FRAMES = 88         # generated frames of the empty mel whose decoded PCM gives the bias (the public denoisers use 88 too)

    def vocoder_bias_pcm(self) -> torch.Tensor:
        """The decoder's answer to an empty mel: VOCODER_BIAS_FRAMES zero frames, no reference part -> int16 [samples] on the device."""
        T = self.VOCODER_BIAS_FRAMES
        x = torch.zeros((1, T, self.spec.n_mel), dtype=torch.float32, device=self.device)
        pre = {"ref_signal_len": torch.zeros((1,), dtype=torch.int32, device=self.device),
               "seq_len": torch.full((1,), T, dtype=torch.int32, device=self.device)}
        pcm, pcm_len = self.decode(x, pre, T)
        return pcm[0, : int(pcm_len[0])].contiguous()

    def vocoder_bias(self) -> torch.Tensor:
        """The bias profile of this engine's decoder, HiFi-GAN or Vocos: pcm_denoise_bias of vocoder_bias_pcm(), float64
        [1][513] on the device.  Computed once per engine: weights and decoder are bound at construction; an option that changes what the
        decoder computes (set_option) drops it."""
        if self._vocoder_bias is None:
            pcm = self.vocoder_bias_pcm()
            self._vocoder_bias = self.pcm_denoise_bias(pcm, [[0, pcm.numel()]])
        return self._vocoder_bias

    def decode_bucketed(self, x: torch.Tensor, pre: Dict[str, torch.Tensor], gen_frames, pad_frac: float = 0.10, min_units: int = 4):
        """The vocoder works on padded [B][C][T_max] planes (the acoustic stages pack ragged rows, the conv stack does not),
        so a ragged batch is decoded in length buckets.  gen_frames: host list of generated frames per item."""
        from .sharding import plan_batches
        B = x.shape[0]
        hop = self.spec.hop_length
        t_max = int(max(gen_frames))
        groups = plan_batches([int(f) for f in gen_frames], B, pad_frac=pad_frac, min_units=min_units)
        if len(groups) == 1:
            return self.decode(x, pre, t_max)
        pcm = torch.zeros((B, t_max * hop), dtype=torch.int16, device=self.device)
        pcm_len = torch.empty((B,), dtype=torch.int32, device=self.device)
        for grp in groups:
            idx = torch.tensor(grp, dtype=torch.int64, device=self.device)
            sub = {"ref_signal_len": pre["ref_signal_len"].index_select(0, idx).contiguous(), "seq_len": pre["seq_len"].index_select(0, idx).contiguous()}
            t_g = int(max(gen_frames[i] for i in grp))
            p, n = self.decode(x.index_select(0, idx).contiguous(), sub, t_g)
            pcm[idx, : t_g * hop] = p
            pcm_len[idx] = n
        return pcm, pcm_len

    # ------------------------------------------------------------------ start noise on the device (N9)
    def noise_keys_device(self, keys) -> torch.Tensor:
        """Philox keys {seed, stream} as the int64 [B][2] device tensor vv_noise_fill reads: from model_spec.noise_keys' numpy uint64
        rows (a 16 * B byte upload), or a device tensor already in that form, which is returned as it is."""
        if isinstance(keys, torch.Tensor):
            assert keys.is_cuda and keys.dtype == torch.int64 and keys.is_contiguous() and keys.dim() == 2 and keys.shape[1] == 2
            return keys
        import numpy as np
        k = np.ascontiguousarray(keys, dtype=np.uint64)
        if k.ndim != 2 or k.shape[1] != 2:
            raise ValueError("noise keys are uint64 [B][2] = {seed, stream} (model_spec.noise_keys)")
        return torch.from_numpy(k.view(np.int64)).to(self.device)

    def noise(self, keys, seq_len: torch.Tensor, N: int, kind: int = 0, n_mel: Optional[int] = None,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The start noise of B items, drawn in HBM (vv_noise_fill): fp32 [B, N, n_mel], item b's rows [0, clamp(seq_len[b], 0, N)) from
        the Philox stream keys[b] = {seed, stream}, +0.0 behind them.  keys: model_spec.noise_keys rows or their device form
        (noise_keys_device); seq_len int32 [B] on the device; kind 0 = normals, 1 = the uniforms under them (exact tests); n_mel defaults
        to the model's; out = an existing [B, N, n_mel] buffer to fill (a captured graph's static one).  Raises on a refused call."""
        kd = self.noise_keys_device(keys)
        B, M = int(kd.shape[0]), int(self.spec.n_mel if n_mel is None else n_mel)
        assert seq_len.is_cuda and seq_len.dtype == torch.int32 and seq_len.is_contiguous() and seq_len.shape == (B,)
        if out is None:
            out = torch.empty((B, int(N), M), dtype=torch.float32, device=self.device)
        assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.shape == (B, int(N), M)
        with self._lock, torch.cuda.device(self.device):
            self._check(self.lib.vv_noise_fill(self.ctx, B, int(N), M, out.data_ptr(), seq_len.data_ptr(), kd.data_ptr(), int(kind),
                                               self._stream()))
        return out

    @staticmethod
    def _one_noise(noise, noise_keys):
        if (noise is None) == (noise_keys is None):
            raise ValueError("give exactly one of noise (a tensor drawn by the caller) and noise_keys (drawn on the device)")

    def synthesize_batch(self, audio, audio_len, text_ids, text_len, seq_len, N: int, noise: Optional[torch.Tensor], t_gen_max: int,
                         n_steps: Optional[int] = None, max_audio_len: Optional[int] = None, gen_frames=None, seq_len_host=None,
                         audio_len_host=None, cfg: Optional[torch.Tensor] = None, guide: Optional[torch.Tensor] = None, noise_keys=None,
                         apg=None, block_cache=None, block_cache_interval=None, cfg_norm=None):
        """Whole hot path for a batch, state resident in HBM: preprocess -> ODE steps -> vocoder.
        noise fp32 [B, N, n_mel] on the device, or None with noise_keys = (model_spec.noise_keys rows): the noise is then drawn on the
        device (``noise``) and nothing of it crosses PCIe.  Exactly one of the two.
        gen_frames (host list, optional): per-item generated frames; lets the vocoder run in length buckets on ragged batches.
        seq_len_host (optional): the lengths on the host too -- the Euler-step call then runs without any stream synchronisation.
        cfg (optional fp32 [B] on the device): per-item guidance strength.  guide (optional uint8 [n_evals, B] on the host): the
        guidance mask of transformer_steps.  apg (optional pair of fp32 [B] device tensors): its projected guidance.  block_cache /
        block_cache_interval (N23): its block caching.  cfg_norm (N24): its CFG-Zero* / rescale pair."""
        self._one_noise(noise, noise_keys)
        pre = self.preprocess(audio, audio_len, text_ids, text_len, seq_len, N, max_audio_len, seq_len_host=seq_len_host,
                              audio_len_host=audio_len_host)
        x = noise.clone() if noise_keys is None else self.noise(noise_keys, seq_len, N)
        self.transformer_steps(x, pre, 0, self.n_steps if n_steps is None else n_steps, cfg=cfg, guide=guide, apg=apg, block_cache=block_cache,
                               block_cache_interval=block_cache_interval, cfg_norm=cfg_norm)
        if gen_frames is not None and len(gen_frames) == x.shape[0]:
            pcm, pcm_len = self.decode_bucketed(x, pre, gen_frames)
            if pcm.shape[1] < t_gen_max * self.spec.hop_length:
                pcm = torch.nn.functional.pad(pcm, (0, t_gen_max * self.spec.hop_length - pcm.shape[1]))
        else:
            pcm, pcm_len = self.decode(x, pre, t_gen_max)
        return x, pcm, pcm_len, pre

    # ------------------------------------------------------------------ speech editing (N5)
    def edit_splice(self, src: torch.Tensor, rows, B: int, ld_out: int) -> torch.Tensor:
        """src int16 [n] on the device (source clips back to back) and rows = HOST rows {item, src_off, dst_off, n} -> int16 [B, ld_out]:
        out[item][dst_off + k] = src[src_off + k], 0 wherever no row writes (ld_out % 4 == 0).  The rows are validated here, on the host,
        before anything is launched: the kernel indexes both buffers by them."""
        assert src.is_cuda and src.dtype == torch.int16 and src.is_contiguous()
        rows = [[int(v) for v in r] for r in rows]
        n_src = src.numel()
        per_item = {}
        for r in rows:
            if len(r) != 4:
                raise ValueError("edit_splice: a descriptor row has 4 entries")
            item, so, do, n = r
            if not (0 <= item < B) or so < 0 or do < 0 or n < 0 or so + n > n_src or do + n > ld_out:
                raise ValueError(f"edit_splice: descriptor row {r} does not fit the buffers ({n_src} source samples, [{B}, {ld_out}] out)")
            per_item.setdefault(item, []).append((do, do + n))
        for spans in per_item.values():
            spans.sort()
            if any(spans[i][0] < spans[i - 1][1] for i in range(1, len(spans))):
                raise ValueError("edit_splice: the rows of one item overlap on the output")
        out = torch.empty((B, ld_out), dtype=torch.int16, device=self.device)
        d = torch.tensor(rows, dtype=torch.int64).reshape(-1, 4).to(self.device)
        with self._lock, torch.cuda.device(self.device):
            self._check(self.lib.vv_edit_splice(self.ctx, src.data_ptr(), n_src, d.data_ptr(), len(rows), B, out.data_ptr(), ld_out,
                                                self._stream()))
        return out

    def preprocess_edit(self, audio: torch.Tensor, audio_len: torch.Tensor, text_ids: torch.Tensor, text_len: torch.Tensor,
                        seq_len: torch.Tensor, N: int, keep: torch.Tensor, audio_len_host, max_audio_len: Optional[int] = None,
                        seq_len_host=None) -> Dict[str, torch.Tensor]:
        """preprocess with the mel conditioning masked by keep (uint8 [B, >= N] on the device): the same ``pre`` dict, ref_signal_len 0."""
        B = audio.shape[0]
        for t, d in ((audio, torch.int16), (audio_len, torch.int32), (text_ids, torch.int32), (text_len, torch.int32), (seq_len, torch.int32),
                     (keep, torch.uint8)):
            assert t.is_cuda and t.dtype == d and t.is_contiguous(), "preprocess_edit inputs must be contiguous device tensors"
        assert keep.dim() == 2 and keep.shape[0] == B
        cat = torch.empty((B, N, self.spec.cond_dim), dtype=torch.float32, device=self.device)
        cat_drop = torch.empty_like(cat)
        ref_len = torch.empty((B,), dtype=torch.int32, device=self.device)
        mal = int(max_audio_len if max_audio_len is not None else audio.shape[1])
        with self._lock, torch.cuda.device(self.device):
            self._check(self.lib.vv_preprocess_edit(self.ctx, B, N, audio.data_ptr(), audio.shape[1], mal, audio_len.data_ptr(), _host_lens(B, audio_len_host),
                                                    text_ids.data_ptr(), text_ids.shape[1], text_len.data_ptr(), seq_len.data_ptr(),
                                                    cat.data_ptr(), cat_drop.data_ptr(), ref_len.data_ptr(), keep.data_ptr(), keep.shape[1],
                                                    self._stream()))
        return self._pre_dict(cat, cat_drop, ref_len, seq_len, N, seq_len_host)

    def edit_restore(self, x: torch.Tensor, pre: Dict[str, torch.Tensor], keep: torch.Tensor) -> torch.Tensor:
        """x fp32 [B,N,n_mel] in place: the kept frames (keep[b][t], t < seq_len[b]) become the conditioning's mel, bit for bit."""
        B, N, M = x.shape
        assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and M == self.spec.n_mel
        assert keep.is_cuda and keep.dtype == torch.uint8 and keep.is_contiguous() and keep.dim() == 2 and keep.shape[0] == B
        with self._lock, torch.cuda.device(self.device):
            self._check(self.lib.vv_edit_restore(self.ctx, B, N, x.data_ptr(), pre["cat_mel_text"].data_ptr(), keep.data_ptr(), keep.shape[1],
                                                 pre["seq_len"].data_ptr(), self._stream()))
        return x

    def edit_batch(self, src: torch.Tensor, rows, spliced_len, text_ids: torch.Tensor, text_len: torch.Tensor, keep: torch.Tensor,
                   noise: Optional[torch.Tensor] = None, n_steps: Optional[int] = None, cfg: Optional[torch.Tensor] = None,
                   guide: Optional[torch.Tensor] = None, noise_keys=None, apg=None, block_cache=None, block_cache_interval=None,
                   cfg_norm=None):
        """B speech edits in one batch: splice -> masked preprocess -> Euler steps -> restore -> vocoder over every frame.
        src int16 [n] (device, the source clips back to back), rows = host splice rows {item, src_off, dst_off, n}, spliced_len = host
        list of the B spliced clip lengths L_b (frames N_b = L_b // hop + 1), text_ids / text_len int32 on the device (the new full
        transcripts), keep uint8 [B, >= max N_b] (device), noise fp32 [B, max N_b, n_mel] (device) or, in its place, noise_keys =
        model_spec.noise_keys rows (drawn on the device; exactly one of the two).  cfg / guide / apg / cfg_norm: as transformer_steps.
        Returns (x, pcm, pcm_len): pcm int16 [B, N * hop] holds the edited clip b in its first pcm_len[b] = min(L_b, the vocoder's
        output of N_b frames) samples -- L_b with the HiFi-GAN (hop * N_b >= L_b), hop * (N_b - 1) with Vocos (the rest is zeros)."""
        s = self.spec
        hop = s.hop_length
        L = [int(v) for v in spliced_len]
        B = len(L)
        frames = [v // hop + 1 for v in L]
        N = max(frames)
        self._one_noise(noise, noise_keys)
        assert noise is None or (noise.shape == (B, N, s.n_mel) and noise.is_cuda and noise.dtype == torch.float32)
        mal = max(max(L), s.n_fft)                  # the audio plane is at least n_fft wide (vv_preprocess's contract)
        audio = self.edit_splice(src, rows, B, (mal + 3) // 4 * 4)
        i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=self.device)
        pre = self.preprocess_edit(audio, i32(L), text_ids, text_len, i32(frames), N, keep, L, max_audio_len=mal, seq_len_host=frames)
        x = noise.clone() if noise_keys is None else self.noise(noise_keys, pre["seq_len"], N)
        self.transformer_steps(x, pre, 0, self.n_steps if n_steps is None else n_steps, cfg=cfg, guide=guide, apg=apg, block_cache=block_cache,
                               block_cache_interval=block_cache_interval, cfg_norm=cfg_norm)
        self.edit_restore(x, pre, keep)
        pcm, _ = self.decode(x, pre, N)
        return x, pcm, i32([min(v, s.pcm_samples(f)) for v, f in zip(L, frames)])

    # ------------------------------------------------------------------ hipGraph-captured vocoder step (config 5)
    def capture_decode(self, B: int, N: int, t_gen_max: int) -> "GraphedDecode":
        """Capture the decode stage (frame slice -> vocoder -> int16) for a fixed shape into a hipGraph.
        Long-form synthesis replays it per chunk group: ~80 launches become one graph launch."""
        return GraphedDecode(self, B, N, t_gen_max)

    def capture_steps(self, B: int, N: int, seq_len_host, t_gen_max: int, device_noise: bool = False) -> "GraphedSteps":
        """Capture all Euler steps + the decode of one batch shape into ONE hipGraph (single-utterance latency path).
        device_noise: the noise fill (vv_noise_fill) is captured in front of the steps and the graph is called with keys."""
        return GraphedSteps(self, B, N, seq_len_host, t_gen_max, device_noise=device_noise)

    # ------------------------------------------------------------------ reference-clip ingest (N3)
    def resample_poly(self, x: torch.Tensor, taps: torch.Tensor, up: int, down: int, skip: int, n_out: int) -> torch.Tensor:
        """x f32 [n_in] and taps f64 [n_taps] on the device -> f32 [n_out]."""
        assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and taps.is_cuda and taps.dtype == torch.float64
        y = torch.empty((n_out,), dtype=torch.float32, device=self.device)
        with self._lock, torch.cuda.device(self.device):
            self._check(self.lib.vv_resample_poly(self.ctx, x.data_ptr(), x.numel(), taps.data_ptr(), taps.numel(), up, down, skip,
                                                  y.data_ptr(), n_out, self._stream()))
        return y

    def ingest_pcm(self, pcm: torch.Tensor, desc, total_out: int) -> torch.Tensor:
        """pcm uint8 [bytes] on the device (the clips' interleaved PCM back to back) and desc = HOST rows of 8 ints per clip
        (include/vvtts.h: byte offset, width, channels, n_frames, src / g, dst / g, out offset, n_out) -> f32 [total_out]: mono samples at
        the destination rate (audioop.tomono + audioop.ratecv arithmetic).  The rows are validated here, on the host, before anything
        is launched: the kernel indexes the byte buffer by them."""
        assert pcm.is_cuda and pcm.dtype == torch.uint8 and pcm.is_contiguous()
        rows = [[int(v) for v in r] for r in desc]
        if not rows:
            raise ValueError("ingest_pcm: no clips")
        for r in rows:
            if len(r) != 8:
                raise ValueError("ingest_pcm: a descriptor row has 8 entries")
            off, width, ch, n_frames, I, O, out_off, n_out = r
            want = n_frames if I == O else ((n_frames - 1) * O // I + 1 if n_frames > 0 else 0)
            if (width not in (1, 2, 4) or ch < 1 or n_frames < 1 or I < 1 or O < 1 or off < 0 or off % width or n_out != want or n_out < 1
                    or off + n_frames * ch * width > pcm.numel() or out_off < 0 or out_off + n_out > total_out):
                raise ValueError(f"ingest_pcm: descriptor row {r} does not fit the buffers ({pcm.numel()} PCM bytes, {total_out} output samples)")
        y = torch.empty((total_out,), dtype=torch.float32, device=self.device)
        d = torch.tensor(rows, dtype=torch.int64).to(self.device)
        with self._lock, torch.cuda.device(self.device):
            self._check(self.lib.vv_ingest_pcm(self.ctx, pcm.data_ptr(), d.data_ptr(), len(rows), max(r[7] for r in rows), y.data_ptr(), self._stream()))
        return y

    def normalize_clips(self, x: torch.Tensor, offsets: torch.Tensor, max_len: int = 0) -> torch.Tensor:
        """x f32 [total] = clips back to back, offsets int64 [n+1] (device) -> int16 [total] (DC removed, peak 29491);
        max_len = the longest clip when the caller knows it (else it is read back from the offsets)."""
        assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and offsets.is_cuda and offsets.dtype == torch.int64
        n = offsets.numel() - 1
        if not max_len:
            oh = offsets.cpu()
            if int(oh[0]) != 0 or int(oh[-1]) != x.numel() or bool((oh[1:] < oh[:-1]).any()):
                raise ValueError("normalize_clips: offsets must run from 0 to x.numel(), non-decreasing")
            max_len = int((oh[1:] - oh[:-1]).max())
        out = torch.empty((x.numel(),), dtype=torch.int16, device=self.device)
        scratch = torch.empty((int(self.lib.vv_normalize_scratch_bytes(n, x.numel())),), dtype=torch.uint8, device=self.device)
        with self._lock, torch.cuda.device(self.device):
            self._check(self.lib.vv_normalize_clips(self.ctx, x.data_ptr(), offsets.data_ptr(), n, int(max_len), scratch.data_ptr(),
                                                    out.data_ptr(), self._stream()))
        return out

    def set_rope_theta(self, theta: float):
        """theta > 1: the rope tables of this engine are the standard ones of that base, the bf16 QKV epilogue computes the angles;
        0: the tables are read (vv_set_rope_theta)."""
        with self._lock:
            self._check(self.lib.vv_set_rope_theta(self.ctx, float(theta)))
            self._rope_theta = float(theta)
            self.grid_generation += 1

    @contextlib.contextmanager
    def reading_rope_tables(self):
        """For ONE caller's calls: the rope tables handed to transformer_steps are read, not recomputed from theta (a session that
        is fed non-standard tables).  Holds the engine lock, so no other call and no graph replay sees the switched mode; the
        previous mode is restored on exit (captured graphs stay valid: none can run in between)."""
        with self._lock:
            prev = self._rope_theta
            self._check(self.lib.vv_set_rope_theta(self.ctx, 0.0))
            try:
                yield
            finally:
                self._check(self.lib.vv_set_rope_theta(self.ctx, prev))

    def set_option(self, name: str, value: int):
        """Context switches of the C ABI (vv_set_option), e.g. ``fuse_mrf`` 0/1."""
        with self._lock:
            self._check(self.lib.vv_set_option(self.ctx, name.encode(), int(value)))
            self.grid_generation += 1
            self._vocoder_bias = None        # N19: an option may change what the decoder computes

    # ------------------------------------------------------------------ profiling
    def prof_enable(self, on: bool):
        self._check(self.lib.vv_prof_enable(self.ctx, 1 if on else 0))

    def prof_collect(self) -> Dict[str, Dict[str, float]]:
        n = len(PROF_CLASSES)
        la, ms, fl, by = (C.c_int64 * n)(), (C.c_double * n)(), (C.c_double * n)(), (C.c_double * n)()
        self._check(self.lib.vv_prof_collect(self.ctx, la, ms, fl, by))
        return {PROF_CLASSES[i]: {"launches": int(la[i]), "ms": float(ms[i]), "flops": float(fl[i]), "bytes": float(by[i])}
                for i in range(n)}


class GraphedDecode:
    """hipGraph replay of the decode stage at a fixed (B, N, t_gen_max).  Static input/output buffers AND the
    stage's whole workspace are owned here (``vv_decode_into``): the captured launches point only into memory
    that lives as long as this object, so later calls that grow the context arena cannot invalidate the graph.
    ``__call__`` copies the state in and replays."""

    def __init__(self, eng: HipSynth, B: int, N: int, t_gen_max: int, ws: Optional[torch.Tensor] = None):
        """ws: optional caller-owned uint8 workspace of at least ``vv_decode_ws_bytes`` bytes (a ``DecodeGraphCache`` shares one
        block between all graphs of an engine: replays are serialised by the engine lock on one stream)."""
        self.eng, self.B, self.N, self.t_gen_max = eng, B, N, t_gen_max
        dev, s = eng.device, eng.spec
        self.x = torch.zeros((B, N, s.n_mel), dtype=torch.float32, device=dev)
        self.ref_len = torch.zeros((B,), dtype=torch.int32, device=dev)
        self.seq_len = torch.full((B,), N, dtype=torch.int32, device=dev)
        self.pcm = torch.zeros((B, t_gen_max * s.hop_length), dtype=torch.int16, device=dev)
        self.pcm_len = torch.zeros((B,), dtype=torch.int32, device=dev)
        nb = C.c_uint64()
        eng._check(eng.lib.vv_decode_ws_bytes(eng.ctx, B, t_gen_max, C.byref(nb)))
        if ws is not None:
            assert ws.is_cuda and ws.dtype == torch.uint8 and ws.numel() >= int(nb.value)
        self.ws = ws if ws is not None else torch.empty((int(nb.value),), dtype=torch.uint8, device=dev)   # torch allocations are 512-byte aligned
        self.ws_need = int(nb.value)
        self._launch()                                   # warm-up: sets kernel attributes before capture
        torch.cuda.synchronize(dev)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self._launch()

    def _launch(self):
        e = self.eng
        with e._lock, torch.cuda.device(e.device):
            e._check(e.lib.vv_decode_into(e.ctx, self.B, self.N, self.x.data_ptr(), self.ref_len.data_ptr(), self.seq_len.data_ptr(),
                                          self.t_gen_max, self.pcm.data_ptr(), self.pcm.shape[1], self.pcm_len.data_ptr(), None,
                                          self.ws.data_ptr(), self.ws.numel(), e._stream()))

    def __call__(self, x: torch.Tensor, ref_len: torch.Tensor, seq_len: torch.Tensor):
        with self.eng._lock:                             # one stream of work per context, replay included
            self.x.copy_(x)
            self.ref_len.copy_(ref_len)
            self.seq_len.copy_(seq_len)
            self.graph.replay()
        return self.pcm, self.pcm_len


    def io_bytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in (self.x, self.ref_len, self.seq_len, self.pcm, self.pcm_len))


class GraphedSteps:
    """ONE hipGraph for the whole ODE integration + decode of a fixed batch shape (B, N, the per-item lengths, t_gen_max): all
    ``n_steps`` Euler steps (``vv_transformer_steps_into``: ~170 launches per step at the full model) and the decode stage
    (``vv_decode_into``) are captured once and replayed as a single graph launch -- the single-utterance latency path, where the ~5,300
    launch-sized kernels of an utterance are bound by launch cadence, not by the kernels.  The row count of every launch is part
    of the captured shapes, so a graph serves exactly one tuple of lengths; static I/O buffers and ONE workspace block (the steps and
    the decode run one after the other on one stream and share it) are owned here.  ``__call__`` copies the inputs in and replays.
    No reference counterpart: the reference pays a host round trip per step (core/tts_engine.py:157-172)."""

    def __init__(self, eng: HipSynth, B: int, N: int, seq_len_host, t_gen_max: int, n_steps: Optional[int] = None, device_noise: bool = False):
        """device_noise (N9): the graph starts with vv_noise_fill into ``x`` from a static key buffer, and ``__call__`` takes the keys
        (model_spec.noise_keys rows) in place of a noise tensor: a replay for a new request uploads 16 bytes per item, no noise."""
        self.eng, self.B, self.N, self.t_gen_max = eng, int(B), int(N), int(t_gen_max)
        self.device_noise = bool(device_noise)
        self.keys = torch.zeros((int(B), 2), dtype=torch.int64, device=eng.device) if self.device_noise else None
        self.seq_host = [int(v) for v in seq_len_host]
        assert len(self.seq_host) == self.B
        self.n_steps = eng.n_steps if n_steps is None else int(n_steps)
        dev, s = eng.device, eng.spec
        self.x = torch.zeros((B, N, s.n_mel), dtype=torch.float32, device=dev)
        self.cat = torch.zeros((B, N, s.cond_dim), dtype=torch.float32, device=dev)
        self.cat_drop = torch.zeros_like(self.cat)
        self.seq_len = torch.tensor(self.seq_host, dtype=torch.int32, device=dev)
        self.ref_len = torch.zeros((B,), dtype=torch.int32, device=dev)
        self.pcm = torch.zeros((B, t_gen_max * s.hop_length), dtype=torch.int16, device=dev)
        self.pcm_len = torch.zeros((B,), dtype=torch.int32, device=dev)
        self._host = _host_lens(B, self.seq_host)
        nb_t, nb_d = eng._steps_ws_bytes(eng.lib.vv_transformer_ws_bytes, B, N, self._host), C.c_uint64()
        eng._check(eng.lib.vv_decode_ws_bytes(eng.ctx, B, t_gen_max, C.byref(nb_d)))
        self.ws = torch.empty((max(nb_t, int(nb_d.value)),), dtype=torch.uint8, device=dev)
        self._launch()                                   # warm-up: sets kernel attributes before capture
        torch.cuda.synchronize(dev)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self._launch()
        # the captured launches hold device pointers into the context's time-grid tables and its step count, rope mode and lane
        # plan: anything that changes those (HipSynth.set_nfe / set_rope_theta / set_option) makes this graph stale
        self.generation = eng.grid_generation

    def stale(self) -> bool:
        return self.generation != self.eng.grid_generation

    def _launch(self):
        e = self.eng
        with e._lock, torch.cuda.device(e.device):
            if self.device_noise:
                e._check(e.lib.vv_noise_fill(e.ctx, self.B, self.N, e.spec.n_mel, self.x.data_ptr(), self.seq_len.data_ptr(), self.keys.data_ptr(),
                                             0, e._stream()))
            e._check(e.lib.vv_transformer_steps_into(e.ctx, self.B, self.N, self.seq_len.data_ptr(), self._host, self.x.data_ptr(),
                                                     self.cat.data_ptr(), self.cat_drop.data_ptr(), e.rope[0].data_ptr(), e.rope[1].data_ptr(),
                                                     e.rope[2].data_ptr(), e.rope[3].data_ptr(), 0, self.n_steps, self.ws.data_ptr(), self.ws.numel(),
                                                     e._stream()))
            e._check(e.lib.vv_decode_into(e.ctx, self.B, self.N, self.x.data_ptr(), self.ref_len.data_ptr(), self.seq_len.data_ptr(),
                                          self.t_gen_max, self.pcm.data_ptr(), self.pcm.shape[1], self.pcm_len.data_ptr(), None,
                                          self.ws.data_ptr(), self.ws.numel(), e._stream()))

    def __call__(self, noise: torch.Tensor, pre: Dict[str, torch.Tensor]):
        """noise [B,N,n_mel] -- with ``device_noise`` the B keys instead -- and ``pre`` (HipSynth.preprocess of the same batch) ->
        (x, pcm, pcm_len): views of the static buffers, valid until the next call."""
        with self.eng._lock:                             # the setters take the same lock: the check and the replay see one state
            if self.stale():
                raise RuntimeError("captured Euler-step graph is stale: the engine's time grid, rope mode or an option changed after the "
                                   "capture (set_nfe / set_rope_theta / set_option); capture again with HipSynth.capture_steps")
            if self.device_noise:
                self.keys.copy_(self.eng.noise_keys_device(noise))
            else:
                self.x.copy_(noise)
            self.cat.copy_(pre["cat_mel_text"])
            self.cat_drop.copy_(pre["cat_mel_text_drop"])
            self.ref_len.copy_(pre["ref_signal_len"])
            self.graph.replay()
        return self.x, self.pcm, self.pcm_len

    def pinned_bytes(self) -> int:
        return self.ws.numel() + sum(t.numel() * t.element_size() for t in (self.x, self.cat, self.cat_drop, self.pcm))


class DecodeGraphCache:
    """Bounded cache of captured decode graphs for one engine, keyed by (B, N, t_gen_max).

    A service with varied voices sees a new generated-frame count per reference clip; unbounded, every key would pin its own
    workspace (5 x B x max(C*T) x 4 B: ~170 MB per item at full size) for the life of the engine.  Here
      * the workspace is ONE block shared by every graph of the cache (replays are serialised by the engine lock on one stream);
        it is replaced by a larger one only when a new key needs more -- graphs captured on the old block keep it alive until
        they are evicted;
      * entries are evicted least-recently-used beyond ``max_entries`` or when the pinned bytes (distinct workspace blocks +
        per-graph I/O buffers) exceed ``max_bytes``;
      * callers bucket the key (``bucket``): N to multiples of 128 frames, t_gen_max to multiples of 64, so that nearby clips and
        chunk lengths share a graph (the decode masks every item by its own lengths).
    """

    def __init__(self, eng: HipSynth, max_entries: int = 8, max_bytes: int = 16 << 30):
        from collections import OrderedDict
        self.eng, self.max_entries, self.max_bytes = eng, max(1, int(max_entries)), int(max_bytes)
        self._graphs: "OrderedDict[Tuple[int, int, int], GraphedDecode]" = OrderedDict()
        self._ws: Optional[torch.Tensor] = None
        self.hits = self.misses = self.evictions = 0

    @staticmethod
    def bucket(N: int, t_gen: int) -> Tuple[int, int]:
        Nb = (int(N) + 127) // 128 * 128
        return Nb, min(Nb, (int(t_gen) + 63) // 64 * 64)

    def pinned_bytes(self) -> int:
        blocks = {g.ws.data_ptr(): g.ws.numel() for g in self._graphs.values()}
        if self._ws is not None:
            blocks[self._ws.data_ptr()] = self._ws.numel()
        return sum(blocks.values()) + sum(g.io_bytes() for g in self._graphs.values())

    def __len__(self):
        return len(self._graphs)

    def __contains__(self, key):
        return key in self._graphs

    def get(self, B: int, N: int, t_gen_max: int) -> GraphedDecode:
        key = (int(B), int(N), int(t_gen_max))
        g = self._graphs.get(key)
        if g is not None:
            self.hits += 1
            self._graphs.move_to_end(key)
            return g
        self.misses += 1
        nb = C.c_uint64()
        self.eng._check(self.eng.lib.vv_decode_ws_bytes(self.eng.ctx, key[0], key[2], C.byref(nb)))
        if self._ws is None or self._ws.numel() < int(nb.value):
            self._ws = torch.empty((int(nb.value),), dtype=torch.uint8, device=self.eng.device)
        g = GraphedDecode(self.eng, *key, ws=self._ws)
        self._graphs[key] = g
        while len(self._graphs) > 1 and (len(self._graphs) > self.max_entries or self.pinned_bytes() > self.max_bytes):
            self._graphs.popitem(last=False)          # least recently used; its graph, I/O buffers (and old block) are released
            self.evictions += 1
        return g

    def clear(self):
        self._graphs.clear()
        self._ws = None
