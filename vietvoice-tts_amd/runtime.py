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
from .model_spec import ODE_MAX_EVALS, ModelSpec, check_apg, guidance_mask, ode_plan

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
    "vv_transformer_steps_ex": (C.c_int, [C.c_void_p, C.POINTER(vv_steps_args), C.c_void_p]),
    "vv_ode_stage": (C.c_int, [C.c_void_p, C.POINTER(vv_ode_stage_args), C.c_void_p]),
    "vv_transformer_steps_guided": (C.c_int, [C.c_void_p, C.POINTER(vv_steps_args), C.c_void_p, C.c_int, C.c_void_p]),
    "vv_transformer_guided_ws_bytes": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_uint64)]),
    "vv_ode_stage_guided": (C.c_int, [C.c_void_p, C.POINTER(vv_ode_stage_args), C.c_void_p, C.c_void_p]),
    "vv_transformer_steps_apg": (C.c_int, [C.c_void_p, C.POINTER(vv_steps_args), C.c_void_p, C.c_int, C.POINTER(vv_apg_args), C.c_void_p]),
    "vv_transformer_apg_ws_bytes": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_uint64)]),
    "vv_apg_coef": (C.c_int, [C.c_void_p, C.POINTER(vv_apg_coef_args), C.c_void_p]),
    "vv_ode_stage_apg": (C.c_int, [C.c_void_p, C.POINTER(vv_ode_stage_args), C.c_void_p, C.POINTER(vv_apg_stage_args), C.c_void_p]),
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
    "vv_pcm_stretch_ws_bytes": (C.c_uint64, [C.c_int]),
    "vv_pcm_stretch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                 C.c_int64, C.c_void_p, C.c_uint64, C.c_void_p]),
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


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _dt(s) -> Tuple[int, torch.dtype]:
    if s in ("bf16", "bfloat16", torch.bfloat16, VV_BF16):
        return VV_BF16, torch.bfloat16
    if s in ("fp32", "f32", "float32", torch.float32, VV_F32):
        return VV_F32, torch.float32
    raise ValueError(f"acoustic dtype must be bf16 or fp32, got {s!r}")


JOIN_MAX_N = 24576            # VV_JOIN_MAX_N of include/vvtts.h: the largest junction vv_join_chunks walks
LOUD_RUN = 128                # VV_LOUD_RUN of include/vvtts.h: samples per independent run of the K-weighting recurrence
_I64_MAX = (1 << 63) - 1


def plan_join(requests, cross_fade_duration: float, sample_rate: int, align: int = 8):
    """The host side of vv_join_chunks: every length is known here, so every junction size, position and final owner is too.
    requests = per request a list of chunks (src_off, len) in joining order.  Returns (chunk rows WITHOUT tab_off resolved: column 5 holds
    n, request rows, joined lengths, sorted distinct n, total output samples); request r's result starts at an ``align``-sample boundary.
    Mirrors AudioProcessor.concatenate_with_crossfade_improved: n = min(int(cross_fade_duration * sample_rate), joined so far, len(next));
    a request of one chunk is copied untouched; an empty chunk inside a longer request is refused (the reference raises on it in
    fix_clipped_audio), and so is an empty request."""
    cf = int(cross_fade_duration * sample_rate) if cross_fade_duration > 0 else 0
    rows, reqs, lens, out_pos = [], [], [], 0
    for r, chunks in enumerate(requests):
        chunks = [(int(a), int(b)) for a, b in chunks]
        if not chunks:
            raise ValueError("join_chunks: a request without chunks")
        c0 = len(rows)
        if len(chunks) == 1:
            so, ln = chunks[0]
            if ln < 0:
                raise ValueError("join_chunks: negative chunk length")
            rows.append([so, ln, 0, 0, _I64_MAX, 0, 0, r])
            total = ln
        else:
            total, pos_n = 0, []
            for k, (so, ln) in enumerate(chunks):
                if ln <= 0:
                    raise ValueError("join_chunks: an empty chunk inside a request of two or more chunks")
                n = min(cf, total, ln) if k else 0
                if n > JOIN_MAX_N:
                    raise ValueError(f"join_chunks: a junction of {n} samples, more than {JOIN_MAX_N}")
                pos_n.append((total - n, n))
                total = total - n + ln
            fin = _I64_MAX
            fins = []
            for P, _n in reversed(pos_n):          # fin_k = the smallest position of a later chunk
                fins.append(fin)
                fin = min(fin, P)
            fins.reverse()
            for (so, ln), (P, n), f in zip(chunks, pos_n, fins):
                rows.append([so, ln, P, n, f, n, 1, r])
        out_pos = -(-out_pos // align) * align
        reqs.append([c0, len(chunks), out_pos, total])
        lens.append(total)
        out_pos += total
    return rows, reqs, lens, sorted({row[3] for row in rows if row[3] > 0}), out_pos


class HipSynth:
    """One GPU's synthesis engine: weights resident in HBM, three device-resident stages.

    flat_weights: optional pre-filled flat uint8 device buffer (e.g. received by RCCL broadcast);
    otherwise ``weights`` (fp32 CPU dict) is packed and uploaded here.
    """

    def __init__(self, spec: ModelSpec, weights: Optional[Dict[str, torch.Tensor]] = None, device: str = "cuda:0",
                 acoustic_dtype="bf16", nfe_step: int = 32, flat_weights: Optional[torch.Tensor] = None, ode_method="euler"):
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
        # the tables this engine hands to the transformer stage are the standard ones of spec.rope_theta: the bf16 model may compute the
        # angles in the QKV epilogue instead of reading them (vv_set_rope_theta; the fp32 model reads the tables either way)
        self.grid_generation = 0         # bumped by whatever a captured Euler-step graph has baked in (time grid, rope mode, options)
        self.set_rope_theta(float(spec.rope_theta))
        self.nfe_step = None
        self.ode_method = None           # the solver of the plan in force: a name of model_spec.ODE_METHODS or a custom tableau (a, b)
        self.set_nfe(nfe_step, ode_method)

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

    def set_nfe(self, nfe_step: int, ode_method="euler"):
        """The sampler's plan (N7): ``nfe_step`` grid points = ``nfe_step - 1`` ODE steps of the explicit Runge-Kutta method
        ``ode_method`` (a name of model_spec.ODE_METHODS, or a tableau (a, b)); ``n_evals`` = stages x steps DiT evaluations."""
        if not isinstance(ode_method, str):
            ode_method = (tuple(tuple(r) for r in ode_method[0]), tuple(ode_method[1]))
        if (nfe_step, ode_method) == (self.nfe_step, self.ode_method):
            return
        if nfe_step < 2:
            raise ValueError("nfe_step must be >= 2")
        plan = ode_plan(nfe_step, self.spec.sway_coef, ode_method)
        n_steps = int(plan.dt.numel())
        if n_steps * plan.s > ODE_MAX_EVALS:
            raise ValueError(f"{n_steps} ODE steps of {plan.s} stages exceed {ODE_MAX_EVALS} evaluations")
        sinus = pack.time_sinus_table(self.spec, plan.t).contiguous()
        dtc = plan.dt.contiguous()
        a = (C.c_double * (plan.s * plan.s))(*[v for r in plan.a for v in r])
        b = (C.c_double * plan.s)(*plan.b)
        with self._lock, torch.cuda.device(self.device):          # under the engine lock: no step call or graph replay runs across the change
            self._check(self.lib.vv_set_ode_plan(self.ctx, sinus.data_ptr(), dtc.data_ptr(), n_steps, plan.s, a, b, self._stream()))
            self.nfe_step = nfe_step
            self.ode_method = ode_method
            self.n_steps = n_steps
            self.n_evals = n_steps * plan.s
            self.plan = plan             # the evaluation times a guidance interval is compared with (guidance_mask)
            self._t_host = (C.c_float * self.n_evals)(*[float(v) for v in plan.t])     # the same times for projected guidance (vv_apg_args.t_host)
            self.grid_generation += 1    # vv_set_ode_plan frees and reallocates the tables a captured step graph points into

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
                host = (C.c_int32 * B)(*[int(v) for v in audio_len_host])
                self._check(self.lib.vv_preprocess_h(self.ctx, B, N, audio.data_ptr(), audio.shape[1], mal, audio_len.data_ptr(), host,
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

    def guidance_mask(self, interval, strengths) -> Optional[torch.Tensor]:
        """model_spec.guidance_mask on the plan in force: the ``guide`` of transformer_steps for a guidance interval (one for every item
        or one per item) and the B strengths (a None strength = the model's); None = every item guided everywhere."""
        return guidance_mask(self.plan, interval, [self.spec.cfg_strength if v is None else v for v in strengths])

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

    def transformer_steps(self, x: torch.Tensor, pre: Dict[str, torch.Tensor], step0: int, n_steps: int, seq_len_host=None,
                          cfg: Optional[torch.Tensor] = None, guide: Optional[torch.Tensor] = None, apg=None) -> torch.Tensor:
        """x fp32 [B,N,n_mel] updated in place on the device.  seq_len_host (optional list / array of the B lengths, the same
        values as pre["seq_len"]): the call then needs no read-back and no stream synchronisation (vv_transformer_steps_h).
        cfg (optional fp32 [B] on the device): the guidance strength of each item (vv_transformer_steps_ex); None = the model's.
        guide (optional uint8 [n_evals, B] on the HOST, N8): guided(b, e) of every evaluation of the plan in force
        (vv_transformer_steps_guided; model_spec.guidance_mask builds it); None = every item guided everywhere.
        apg (optional pair (eta, norm) of fp32 [B] device tensors, either None, N11): projected guidance per item
        (vv_transformer_steps_apg; apg_tensors builds it); None, or a pair of Nones = off: the existing entries."""
        B, N, M = x.shape
        assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and M == self.spec.n_mel
        if seq_len_host is None:
            seq_len_host = pre.get("seq_len_host")
        if apg is not None and apg[0] is None and apg[1] is None:
            apg = None
        if cfg is not None or guide is not None or apg is not None:
            assert cfg is None or (cfg.is_cuda and cfg.dtype == torch.float32 and cfg.is_contiguous() and cfg.shape == (B,)), "cfg: fp32 [B] on the device"
            host = None if seq_len_host is None else (C.c_int32 * B)(*[int(v) for v in seq_len_host])
            self.transformer_steps_ex(x, pre, step0, n_steps, host, cfg, guide=guide, apg=apg)
            return x
        with self._lock, torch.cuda.device(self.device):
            tail = (pre["cat_mel_text"].data_ptr(), pre["cat_mel_text_drop"].data_ptr(), pre["rope_cos_q"].data_ptr(), pre["rope_sin_q"].data_ptr(),
                    pre["rope_cos_k"].data_ptr(), pre["rope_sin_k"].data_ptr(), step0, n_steps, self._stream())
            if seq_len_host is not None:
                host = (C.c_int32 * B)(*[int(v) for v in seq_len_host])
                assert len(host) == B
                self._check(self.lib.vv_transformer_steps_h(self.ctx, B, N, pre["seq_len"].data_ptr(), host, x.data_ptr(), *tail))
            else:
                self._check(self.lib.vv_transformer_steps(self.ctx, B, N, pre["seq_len"].data_ptr(), x.data_ptr(), *tail))
        return x

    def guided_ws_bytes(self, B: int, N: int, seq_len_host) -> int:
        """Bytes of a caller-owned workspace for a call with a guidance mask (vv_transformer_guided_ws_bytes; the same for every mask)."""
        host = (C.c_int32 * B)(*[int(v) for v in seq_len_host])
        nb = C.c_uint64()
        with self._lock:
            self._check(self.lib.vv_transformer_guided_ws_bytes(self.ctx, int(B), int(N), host, C.byref(nb)))
        return int(nb.value)

    def apg_ws_bytes(self, B: int, N: int, seq_len_host) -> int:
        """Bytes of a caller-owned workspace for a call with projected guidance (vv_transformer_apg_ws_bytes; the same with any mask)."""
        host = (C.c_int32 * B)(*[int(v) for v in seq_len_host])
        nb = C.c_uint64()
        with self._lock:
            self._check(self.lib.vv_transformer_apg_ws_bytes(self.ctx, int(B), int(N), host, C.byref(nb)))
        return int(nb.value)

    def transformer_steps_ex(self, x: torch.Tensor, pre: Dict[str, torch.Tensor], step0: int, n_steps: int, host=None,
                             cfg: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None,
                             guide: Optional[torch.Tensor] = None, apg=None) -> None:
        """The struct-argument entry as it is (vv_transformer_steps_ex); raises on a non-zero code.  host: a ctypes int32 array of
        the B lengths or None (read back); ws: an optional caller-owned uint8 workspace (needs host).  guide: a contiguous uint8
        HOST tensor [n_evals of the plan in force, ld_guide], handed to vv_transformer_steps_guided as it is (the library checks
        ld_guide >= B).  apg: None, or a pair (eta, norm) of fp32 [B] device tensors (either None), handed to
        vv_transformer_steps_apg with the times of the plan in force."""
        B = x.shape[0]
        if apg is not None:
            if len(apg) != 2 or any(t is not None and not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32
                                                           and t.is_contiguous() and t.shape == (B,)) for t in apg):
                raise ValueError("apg must be a pair (eta, norm) of fp32 [B] device tensors or Nones")
        if guide is not None:
            if not (isinstance(guide, torch.Tensor) and guide.device.type == "cpu" and guide.dtype == torch.uint8 and guide.dim() == 2
                    and guide.is_contiguous() and guide.shape[0] == self.n_evals):
                raise ValueError(f"guide must be a contiguous uint8 host tensor [{self.n_evals} evaluations, >= B]")
        B, N, _ = x.shape
        a = vv_steps_args()
        a.B, a.N, a.seq_len, a.x = B, N, pre["seq_len"].data_ptr(), x.data_ptr()
        a.seq_len_host = None if host is None else C.cast(host, C.c_void_p)
        a.cat_mel_text, a.cat_mel_text_drop = pre["cat_mel_text"].data_ptr(), pre["cat_mel_text_drop"].data_ptr()
        a.rope_cos_q, a.rope_sin_q = pre["rope_cos_q"].data_ptr(), pre["rope_sin_q"].data_ptr()
        a.rope_cos_k, a.rope_sin_k = pre["rope_cos_k"].data_ptr(), pre["rope_sin_k"].data_ptr()
        a.step0, a.n_steps = int(step0), int(n_steps)
        if ws is not None:
            a.ws, a.ws_bytes = ws.data_ptr(), ws.numel()
        a.cfg_item = _ptr(cfg)
        with self._lock, torch.cuda.device(self.device):
            if apg is not None:
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
                         apg=None):
        """Whole hot path for a batch, state resident in HBM: preprocess -> ODE steps -> vocoder.
        noise fp32 [B, N, n_mel] on the device, or None with noise_keys = (model_spec.noise_keys rows): the noise is then drawn on the
        device (``noise``) and nothing of it crosses PCIe.  Exactly one of the two.
        gen_frames (host list, optional): per-item generated frames; lets the vocoder run in length buckets on ragged batches.
        seq_len_host (optional): the lengths on the host too -- the Euler-step call then runs without any stream synchronisation.
        cfg (optional fp32 [B] on the device): per-item guidance strength.  guide (optional uint8 [n_evals, B] on the host): the
        guidance mask of transformer_steps.  apg (optional pair of fp32 [B] device tensors): its projected guidance."""
        self._one_noise(noise, noise_keys)
        pre = self.preprocess(audio, audio_len, text_ids, text_len, seq_len, N, max_audio_len, seq_len_host=seq_len_host,
                              audio_len_host=audio_len_host)
        x = noise.clone() if noise_keys is None else self.noise(noise_keys, seq_len, N)
        self.transformer_steps(x, pre, 0, self.n_steps if n_steps is None else n_steps, cfg=cfg, guide=guide, apg=apg)
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
        host = (C.c_int32 * B)(*[int(v) for v in audio_len_host])
        with self._lock, torch.cuda.device(self.device):
            self._check(self.lib.vv_preprocess_edit(self.ctx, B, N, audio.data_ptr(), audio.shape[1], mal, audio_len.data_ptr(), host,
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
                   guide: Optional[torch.Tensor] = None, noise_keys=None, apg=None):
        """B speech edits in one batch: splice -> masked preprocess -> Euler steps -> restore -> vocoder over every frame.
        src int16 [n] (device, the source clips back to back), rows = host splice rows {item, src_off, dst_off, n}, spliced_len = host
        list of the B spliced clip lengths L_b (frames N_b = L_b // hop + 1), text_ids / text_len int32 on the device (the new full
        transcripts), keep uint8 [B, >= max N_b] (device), noise fp32 [B, max N_b, n_mel] (device) or, in its place, noise_keys =
        model_spec.noise_keys rows (drawn on the device; exactly one of the two).  cfg / guide / apg: as transformer_steps.
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
        self.transformer_steps(x, pre, 0, self.n_steps if n_steps is None else n_steps, cfg=cfg, guide=guide, apg=apg)
        self.edit_restore(x, pre, keep)
        pcm, _ = self.decode(x, pre, N)
        return x, pcm, i32([min(v, s.pcm_samples(f)) for v, f in zip(L, frames)])

    # ------------------------------------------------------------------ the output stage (N10): join, output rate, G.711
    def _fade_tables(self, ns):
        """c = cos(linspace(0, pi / 2, n)) ** 2 | s = sin(..) ** 2 per distinct n, computed by numpy on the HOST (the expression of the
        reference's mix) and kept in one float64 device buffer: -> (buffer, {n: offset in doubles})."""
        import numpy as np
        cache = self.__dict__.setdefault("_fade_cache", {"off": {}, "host": [], "dev": None, "size": 0})
        new = [n for n in ns if n not in cache["off"]]
        if new:
            if cache["size"] + 2 * sum(new) > (1 << 22):       # 32 MB of tables: start over
                cache.update(off={}, host=[], dev=None, size=0)
                new = list(ns)
            for n in new:
                theta = np.linspace(0, np.pi / 2, n)
                cache["off"][n] = cache["size"]
                cache["host"] += [np.cos(theta) ** 2, np.sin(theta) ** 2]
                cache["size"] += 2 * n
            cache["dev"] = torch.from_numpy(np.concatenate(cache["host"])).to(self.device)
        if cache["dev"] is None:
            cache["dev"] = torch.zeros(2, dtype=torch.float64, device=self.device)
        return cache["dev"], cache["off"]

    def join_chunks(self, pcm: torch.Tensor, requests, cross_fade_duration: float, sample_rate: int, out: Optional[torch.Tensor] = None,
                    out_base: int = 0):
        """AudioProcessor.concatenate_with_crossfade_improved for R requests in one call (vv_join_chunks), bit for bit.
        pcm int16 on the device (vv_decode's plane, taken flat); requests = per request the (src_off, len) spans of its chunks in joining
        order.  -> (out int16 flat, offsets, lengths): request r is out[offsets[r] : offsets[r] + lengths[r]].  out (optional) = an
        existing flat int16 buffer, the results then start out_base samples into it (out_base % 8 == 0).  The rows are planned and
        validated here, on the host, before anything is launched; the call never synchronises."""
        assert pcm.is_cuda and pcm.dtype == torch.int16 and pcm.is_contiguous()
        n_pcm = pcm.numel()
        rows, reqs, lens, ns, total = plan_join(requests, cross_fade_duration, sample_rate)
        if out_base < 0 or out_base % 8:
            raise ValueError("join_chunks: out_base must be a non-negative multiple of 8 samples")
        for row in rows:
            if row[0] < 0 or row[0] + row[1] > n_pcm:
                raise ValueError(f"join_chunks: chunk ({row[0]}, {row[1]}) does not fit the {n_pcm} samples of pcm")
        if total + out_base >= 1 << 40 or len(rows) > 65535:
            raise ValueError("join_chunks: too many chunks or samples for one call")
        if out is None:
            out = torch.empty((max(total + out_base, 8),), dtype=torch.int16, device=self.device)
        assert out.is_cuda and out.dtype == torch.int16 and out.is_contiguous() and out.dim() == 1
        if out.numel() < total + out_base:
            raise ValueError(f"join_chunks: out holds {out.numel()} samples, {total + out_base} are needed")
        fade, off = self._fade_tables(ns)
        for row in rows:
            row[5] = off[row[3]] if row[3] > 0 else 0
        for rq in reqs:
            rq[2] += out_base
        rows_h, reqs_h = torch.tensor(rows, dtype=torch.int64).reshape(-1, 8), torch.tensor(reqs, dtype=torch.int64).reshape(-1, 4)
        rows_d, reqs_d = rows_h.to(self.device), reqs_h.to(self.device)
        ws = torch.empty((2 * len(rows),), dtype=torch.int32, device=self.device)
        with self._lock, torch.cuda.device(self.device):
            self._check(self.lib.vv_join_chunks(self.ctx, pcm.data_ptr(), n_pcm, rows_d.data_ptr(), rows_h.data_ptr(), len(rows),
                                                reqs_d.data_ptr(), reqs_h.data_ptr(), len(reqs), fade.data_ptr(), fade.numel(), max(ns, default=0), max(r[1] for r in rows), out.data_ptr(),
                                                out.numel(), ws.data_ptr(), self._stream()))
        return out, [rq[2] for rq in reqs], lens

    def _output_taps(self, src: int, dst: int):
        from .core.audio_processor import output_design
        cache = self.__dict__.setdefault("_out_taps", {})
        if (src, dst) not in cache:
            taps, up, down, skip = output_design(src, dst)
            cache[(src, dst)] = (torch.from_numpy(taps).to(self.device), up, down, skip)
        return cache[(src, dst)]

    def pcm_resample(self, x: torch.Tensor, rows, src: int, dst: int, n_y: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Output rate (vv_pcm_resample): x int16 flat on the device at ``src`` Hz, rows = HOST rows {src_off, n_in, dst_off, n_out, m0, i0}
        (include/vvtts.h) -> int16 [n_y] at ``dst`` Hz through voice_bank.resample_design(src, dst).  A whole clip is m0 = i0 = 0 and
        n_out = ceil(n_in * up / down).  The rows are validated here (in range of both buffers, disjoint on the output).
        out (optional) = an existing flat int16 device buffer to write into (n_y = its length); what the rows read must not be written."""
        assert x.is_cuda and x.dtype == torch.int16 and x.is_contiguous()
        if int(src) == int(dst):
            raise ValueError("pcm_resample: equal rates need no launch")
        taps, up, down, skip = self._output_taps(int(src), int(dst))
        rows = [[int(v) for v in r] for r in rows]
        if not rows or any(len(r) != 6 for r in rows):
            raise ValueError("pcm_resample: rows of 6 entries {src_off, n_in, dst_off, n_out, m0, i0}")
        n_x = x.numel()
        if out is not None:
            assert out.is_cuda and out.dtype == torch.int16 and out.is_contiguous() and out.dim() == 1
            n_y = out.numel()
        n_y = max((r[2] + r[3] for r in rows), default=0) if n_y is None else int(n_y)
        spans = []
        for so, n_in, do, n_out, m0, i0 in rows:
            if min(so, n_in, do, n_out, m0, i0) < 0 or so + n_in > n_x or do + n_out > n_y or (m0 + n_out + skip) * down >= 1 << 62:
                raise ValueError(f"pcm_resample: row {[so, n_in, do, n_out, m0, i0]} does not fit the buffers ({n_x} in, {n_y} out)")
            spans.append((do, do + n_out))
        spans.sort()
        if any(spans[i][0] < spans[i - 1][1] for i in range(1, len(spans))):
            raise ValueError("pcm_resample: rows overlap on the output")
        y = torch.empty((max(n_y, 1),), dtype=torch.int16, device=self.device) if out is None else out
        d = torch.tensor(rows, dtype=torch.int64).reshape(-1, 6).to(self.device)
        with self._lock, torch.cuda.device(self.device):
            self._check(self.lib.vv_pcm_resample(self.ctx, x.data_ptr(), n_x, d.data_ptr(), len(rows), max(r[3] for r in rows), taps.data_ptr(),
                                                 taps.numel(), up, down, skip, y.data_ptr(), n_y, self._stream()))
        return y[:n_y]

    def pcm_encode(self, x: torch.Tensor, rows, encoding: str, n_y: Optional[int] = None) -> torch.Tensor:
        """G.711 (vv_pcm_encode): x int16 flat on the device, rows = HOST rows {src_off, n, dst_off} -> uint8 [n_y]; encoding "ulaw" | "alaw",
        bit-exact to audioop.lin2ulaw / lin2alaw at width 2.  The rows are validated here."""
        assert x.is_cuda and x.dtype == torch.int16 and x.is_contiguous()
        kind = {"ulaw": 1, "alaw": 2}.get(encoding)
        if kind is None:
            raise ValueError("pcm_encode: encoding is 'ulaw' or 'alaw'")
        rows = [[int(v) for v in r] for r in rows]
        if not rows or any(len(r) != 3 for r in rows):
            raise ValueError("pcm_encode: rows of 3 entries {src_off, n, dst_off}")
        n_x = x.numel()
        n_y = max((r[2] + r[1] for r in rows), default=0) if n_y is None else int(n_y)
        spans = []
        for so, n, do in rows:
            if min(so, n, do) < 0 or so + n > n_x or do + n > n_y:
                raise ValueError(f"pcm_encode: row {[so, n, do]} does not fit the buffers ({n_x} in, {n_y} out)")
            spans.append((do, do + n))
        spans.sort()
        if any(spans[i][0] < spans[i - 1][1] for i in range(1, len(spans))):
            raise ValueError("pcm_encode: rows overlap on the output")
        y = torch.empty((max(n_y, 8),), dtype=torch.uint8, device=self.device)
        d = torch.tensor(rows, dtype=torch.int64).reshape(-1, 3).to(self.device)
        with self._lock, torch.cuda.device(self.device):
            self._check(self.lib.vv_pcm_encode(self.ctx, x.data_ptr(), n_x, d.data_ptr(), len(rows), max(r[1] for r in rows), kind,
                                               y.data_ptr(), n_y, self._stream()))
        return y[:n_y]

    # ------------------------------------------------------------------ loudness normalisation (N12)
    def _loudness_tables(self, sr: int) -> torch.Tensor:
        from .core.audio_processor import loudness_tables
        cache = self.__dict__.setdefault("_loud_tables", {})
        if int(sr) not in cache:
            cache[int(sr)] = torch.from_numpy(loudness_tables(int(sr)).copy()).to(self.device)
        return cache[int(sr)]

    def pcm_loudness(self, x: torch.Tensor, rows, sr: int, targets, peak_dbfs: float = -1.0, out: Optional[torch.Tensor] = None,
                     stats: bool = False):
        """Loudness normalisation of R joined signals in one call (vv_pcm_loudness), bit for bit
        core.audio_processor.normalize_loudness.  x int16 flat on the device at ``sr`` Hz; rows = HOST rows (src_off, n, dst_off);
        targets = one LUFS value, or per request a value or None (None = measured, copied through unchanged); peak_dbfs = the sample-peak
        ceiling.  out = None: a new buffer; out = "measure": nothing is written; out = a flat int16 device tensor (x itself with
        dst_off == src_off = in place).  -> the output (None when measuring), and with ``stats`` also the R x 4 float64 DEVICE tensor
        {zbar, kept, P, g}.  The rows are validated here; the call never synchronises."""
        from .core.audio_processor import check_loudness, loudness_ceiling, loudness_target
        assert x.is_cuda and x.dtype == torch.int16 and x.is_contiguous() and x.dim() == 1
        sr = int(sr)
        if sr % 10 or sr // 10 < LOUD_RUN:
            raise ValueError(f"pcm_loudness: the sample rate must be a multiple of 10 Hz and at least {10 * LOUD_RUN} Hz, got {sr}")
        sub = sr // 10
        rows = [[int(v) for v in r] for r in rows]
        if not rows or any(len(r) != 3 for r in rows) or len(rows) > 65535:
            raise ValueError("pcm_loudness: 1 to 65535 rows of 3 entries {src_off, n, dst_off}")
        R = len(rows)
        if not isinstance(targets, (list, tuple)):
            targets = [targets] * R
        if len(targets) != R:
            raise ValueError("pcm_loudness: one target per row")
        par = []
        for t in targets:
            t, pk = check_loudness(t, peak_dbfs)
            par.append([loudness_target(t), loudness_ceiling(pk)])
        measure = isinstance(out, str) and out == "measure"
        n_x = x.numel()
        rps = -(-sub // LOUD_RUN)
        full, runs, spans = [], 0, []
        for so, n, do in rows:
            if min(so, n, do) < 0 or so + n > n_x:
                raise ValueError(f"pcm_loudness: row {[so, n, do]} does not fit the {n_x} samples of x")
            full.append([so, n, do, runs])
            runs += (n // sub) * rps + -(-(n % sub) // LOUD_RUN)
            spans.append((do, do + n))
        y = None
        if not measure:
            n_y = max(e for _b, e in spans)
            if out is None:
                y = torch.empty((max(n_y, 4),), dtype=torch.int16, device=self.device)
            else:
                y = out
                assert y.is_cuda and y.dtype == torch.int16 and y.is_contiguous() and y.dim() == 1
            if y.numel() < n_y:
                raise ValueError(f"pcm_loudness: out holds {y.numel()} samples, {n_y} are needed")
            spans.sort()
            if any(spans[i][0] < spans[i - 1][1] for i in range(1, len(spans))):
                raise ValueError("pcm_loudness: rows overlap on the output")
            if y.data_ptr() == x.data_ptr() and any(r[0] != r[2] for r in rows):
                raise ValueError("pcm_loudness: in place needs dst_off == src_off")
        rows_h = torch.tensor(full, dtype=torch.int64).reshape(-1, 4)
        rows_d = rows_h.to(self.device)
        par_d = torch.tensor(par, dtype=torch.float64).reshape(-1, 2).to(self.device)
        st = torch.empty((R, 4), dtype=torch.float64, device=self.device)
        ws_bytes = int(self.lib.vv_pcm_loudness_ws_bytes(runs, R))
        ws = torch.empty((ws_bytes // 8 + 1,), dtype=torch.float64, device=self.device)
        with self._lock, torch.cuda.device(self.device):
            self._check(self.lib.vv_pcm_loudness(self.ctx, x.data_ptr(), n_x, rows_d.data_ptr(), rows_h.data_ptr(), R, sub,
                                                 self._loudness_tables(sr).data_ptr(), par_d.data_ptr(), _ptr(y), 0 if y is None else y.numel(),
                                                 st.data_ptr(), ws.data_ptr(), ws.numel() * 8, self._stream()))
        return (y, st) if stats else y

    # ------------------------------------------------------------------ look-ahead peak limiter (N13)
    def _limiter_tables(self, L: int):
        """(window, taps, tile) for a look-ahead: the host's float64 tables on the device, cached per L."""
        from .core.audio_processor import limiter_taps, limiter_window
        cache = self.__dict__.setdefault("_limit_tables", {})
        if int(L) not in cache:
            cache[int(L)] = (torch.from_numpy(limiter_window(int(L)).copy()).to(self.device),
                             torch.from_numpy(limiter_taps().copy()).to(self.device), int(self.lib.vv_pcm_limit_tile(int(L))))
        return cache[int(L)]

    def pcm_limit(self, x: torch.Tensor, rows, sr: int, peak_dbfs: float = -1.0, mode: str = "true", gain=1.0, meas: Optional[torch.Tensor] = None,
                  targets=None, L: Optional[int] = None, out=None, stats: bool = False):
        """The look-ahead limiter on R joined signals in one call (vv_pcm_limit), bit for bit
        core.audio_processor.limit_peaks.  x int16 flat on the device at ``sr`` Hz; rows = HOST rows (src_off, n, dst_off) or
        (src_off, n, dst_off, out_lo, out_n): the limiter runs over the row's n samples as a whole signal and y[out_lo, +out_n) of it is
        written at dst_off.  mode "sample" | "true"; peak_dbfs = the ceiling; gain = the pre-gain (one value or one per row).
        meas = the R x 4 device tensor of a pcm_loudness(out="measure", stats=True) call on the same rows, with targets = one LUFS value
        or per row a value or None: rows with a target take the uncapped loudness gain from meas on the device, the others ``gain``.
        L = the look-ahead in samples (None = 5 ms).  out = None: a new buffer; "measure": nothing is written; a flat int16 device tensor
        (x itself with dst_off == src_off + out_lo = in place).  -> the output (None when measuring), and with ``stats`` also the R x 4
        float64 DEVICE tensor {g, e_max, s_min, n_limited}.  The rows are validated here; the call never synchronises."""
        from .core.audio_processor import (LIMITER_MODES, _check_lookahead, check_limiter, check_loudness, limiter_lookahead, loudness_ceiling,
                                           loudness_target)
        assert x.is_cuda and x.dtype == torch.int16 and x.is_contiguous() and x.dim() == 1
        if check_limiter(mode) is None:
            raise ValueError("pcm_limit: a mode is needed")
        L = limiter_lookahead(sr) if L is None else _check_lookahead(L)
        rows = [[int(v) for v in r] for r in rows]
        if not rows or any(len(r) not in (3, 5) for r in rows) or len(rows) > 65535:
            raise ValueError("pcm_limit: 1 to 65535 rows of 3 entries {src_off, n, dst_off} or 5 {src_off, n, dst_off, out_lo, out_n}")
        rows = [r if len(r) == 5 else [r[0], r[1], r[2], 0, r[1]] for r in rows]
        R = len(rows)
        if not isinstance(targets, (list, tuple)):
            targets = [targets] * R
        gains = list(gain) if isinstance(gain, (list, tuple)) else [gain] * R
        if len(targets) != R or len(gains) != R:
            raise ValueError("pcm_limit: one target and one gain per row")
        if meas is None and any(t is not None for t in targets):
            raise ValueError("pcm_limit: a loudness target needs meas, the stats of a pcm_loudness measure call")
        if meas is not None:
            assert meas.is_cuda and meas.dtype == torch.float64 and meas.is_contiguous() and tuple(meas.shape) == (R, 4)
        c = loudness_ceiling(check_loudness(None, peak_dbfs)[1])
        par = []
        for t, g0 in zip(targets, gains):
            if isinstance(g0, bool) or not isinstance(g0, (int, float)) or not 0.0 < float(g0) < float("inf"):
                raise ValueError("pcm_limit: the gain must be a positive finite number")
            par.append([loudness_target(check_loudness(t, peak_dbfs)[0]), c, float(g0)])
        window, taps, tile = self._limiter_tables(L)
        measure = isinstance(out, str) and out == "measure"
        n_x = x.numel()
        samples, tiles, spans = 0, 0, []
        for so, n, do, lo, on in rows:
            if min(so, n, do, lo, on) < 0 or so + n > n_x or lo + on > n:
                raise ValueError(f"pcm_limit: row {[so, n, do, lo, on]} does not fit the {n_x} samples of x or its own n")
            samples += n
            tiles += -(-n // tile)
            if on:
                spans.append((do, do + on))
        y = None
        if not measure:
            n_y = max((e for _b, e in spans), default=0)
            if out is None:
                y = torch.empty((max(n_y, 4),), dtype=torch.int16, device=self.device)
            else:
                y = out
                assert y.is_cuda and y.dtype == torch.int16 and y.is_contiguous() and y.dim() == 1
            if y.numel() < n_y:
                raise ValueError(f"pcm_limit: out holds {y.numel()} samples, {n_y} are needed")
            spans.sort()
            if any(spans[i][0] < spans[i - 1][1] for i in range(1, len(spans))):
                raise ValueError("pcm_limit: rows overlap on the output")
            if y.data_ptr() == x.data_ptr() and any(r[4] and r[2] != r[0] + r[3] for r in rows):
                raise ValueError("pcm_limit: in place needs dst_off == src_off + out_lo")
        rows_h = torch.tensor(rows, dtype=torch.int64).reshape(-1, 5)
        rows_d = rows_h.to(self.device)
        par_d = torch.tensor(par, dtype=torch.float64).reshape(-1, 3).to(self.device)
        st = torch.empty((R, 4), dtype=torch.float64, device=self.device)
        ws_bytes = int(self.lib.vv_pcm_limit_ws_bytes(samples, tiles, R))
        ws = torch.empty((ws_bytes // 8 + 1,), dtype=torch.float64, device=self.device)
        with self._lock, torch.cuda.device(self.device):
            self._check(self.lib.vv_pcm_limit(self.ctx, x.data_ptr(), n_x, rows_d.data_ptr(), rows_h.data_ptr(), R, L, LIMITER_MODES.index(mode),
                                              window.data_ptr(), taps.data_ptr(), par_d.data_ptr(), _ptr(meas), _ptr(y),
                                              0 if y is None else y.numel(), st.data_ptr(), ws.data_ptr(), ws.numel() * 8, self._stream()))
        return (y, st) if stats else y

    def limiter_stream_backend(self, sr: int, peak_dbfs: float = -1.0, mode: str = "true", L: Optional[int] = None):
        """The ``backend(hist, out_lo, out_n)`` callable of core.audio_processor.LimiterStream on this device: the block and its context go
        up, vv_pcm_limit runs over them as one signal and writes the window alone, which comes back."""
        import numpy as np

        def backend(hist, out_lo, out_n):
            hist = np.ascontiguousarray(hist, dtype=np.int16).reshape(-1)
            if out_n <= 0:
                return np.zeros(0, np.int16)
            y = self.pcm_limit(torch.from_numpy(hist).to(self.device), [[0, hist.size, 0, int(out_lo), int(out_n)]], sr, peak_dbfs, mode, L=L)
            return y[: int(out_n)].cpu().numpy()

        return backend

    # ------------------------------------------------------------------ pitch and tempo (N14)
    def pcm_stretch(self, x: torch.Tensor, rows, out: Optional[torch.Tensor] = None):
        """The WSOLA time stretch on R joined signals in one call (vv_pcm_stretch), bit for bit
        core.audio_processor.time_stretch.  x int16 flat on the device; rows = HOST rows (src_off, n, dst_off, p, q): x[src_off, +n) is
        stretched by p / q to ceil(n p / q) samples at dst_off.  out = None: a new buffer; "positions": the search alone, no sample is
        written and y is None; or a flat int16 device tensor that does not overlap x.  -> (y, pos, pos_offs): pos is the int32 device tensor of every frame position, request r's pos_0 ... pos_M are
        pos[pos_offs[r] : pos_offs[r + 1]].  The rows are validated here; the call never synchronises."""
        from .core.audio_processor import WSOLA_HS, check_stretch_ratio, wsola_window
        assert x.is_cuda and x.dtype == torch.int16 and x.is_contiguous() and x.dim() == 1
        rows = [[int(v) for v in r] for r in rows]
        if not rows or any(len(r) != 5 for r in rows) or len(rows) > 65535:
            raise ValueError("pcm_stretch: 1 to 65535 rows of 5 entries {src_off, n, dst_off, p, q}")
        n_x, spans, full, pos_offs = x.numel(), [], [], [0]
        for so, n, do, p, q in rows:
            check_stretch_ratio(p, q)
            if min(so, n, do) < 0 or so + n > n_x or n > 1 << 30:
                raise ValueError(f"pcm_stretch: row {[so, n, do, p, q]} does not fit the {n_x} samples of x")
            n_s = -(-n * p // q)
            if n_s:
                spans.append((do, do + n_s))
            full.append([so, n, do, p, q, pos_offs[-1]])
            pos_offs.append(pos_offs[-1] + -(-n_s // WSOLA_HS) + 1)
        n_y, y = max((e for _b, e in spans), default=0), None
        if not (isinstance(out, str) and out == "positions"):
            if out is None:
                y = torch.empty((max(n_y, 4),), dtype=torch.int16, device=self.device)
            else:
                y = out
                assert y.is_cuda and y.dtype == torch.int16 and y.is_contiguous() and y.dim() == 1
            if y.numel() < n_y:
                raise ValueError(f"pcm_stretch: out holds {y.numel()} samples, {n_y} are needed")
            spans.sort()
            if any(spans[i][0] < spans[i - 1][1] for i in range(1, len(spans))):
                raise ValueError("pcm_stretch: rows overlap on the output")
            if y.data_ptr() < x.data_ptr() + 2 * n_x and x.data_ptr() < y.data_ptr() + 2 * y.numel():
                raise ValueError("pcm_stretch: out overlaps x (the stretch is not in place)")
        if "_wsola_window" not in self.__dict__:
            self._wsola_window = torch.from_numpy(wsola_window().copy()).to(self.device)
        R = len(full)
        rows_h = torch.tensor(full, dtype=torch.int64).reshape(-1, 6)
        rows_d = rows_h.to(self.device)
        pos = torch.empty((pos_offs[-1],), dtype=torch.int32, device=self.device)
        ws = torch.empty((int(self.lib.vv_pcm_stretch_ws_bytes(R)) // 8 + 1,), dtype=torch.int64, device=self.device)
        with self._lock, torch.cuda.device(self.device):
            self._check(self.lib.vv_pcm_stretch(self.ctx, x.data_ptr(), n_x, rows_d.data_ptr(), rows_h.data_ptr(), R, self._wsola_window.data_ptr(),
                                                _ptr(y), 0 if y is None else y.numel(), pos.data_ptr(), pos.numel(), ws.data_ptr(), ws.numel() * 8,
                                                self._stream()))
        return y, pos, pos_offs

    def _prosody(self, buf: torch.Tensor, offs, lens, pitch, tempo):
        """The prosody step of finish_output: -> (new buffer, offsets, lengths).  Every request gets its place in a new buffer, on 8-sample
        boundaries as in plan_join: a request with a stretch alone is stretched into it, one with a pitch is stretched into an
        intermediate region behind it and converted from there (one vv_pcm_resample call per distinct pitch ratio), one without prosody
        is copied sample for sample."""
        from .core.audio_processor import prosody_plan
        R = len(lens)
        plans = [prosody_plan(lens[i], pitch[i], tempo[i]) for i in range(R)]
        new_offs, new_lens, end = [], [], 0
        for i in range(R):
            end = -(-end // 8) * 8
            new_offs.append(end)
            new_lens.append(lens[i] if plans[i] is None else plans[i].n_f)
            end += new_lens[i]
        base = -(-end // 8) * 8
        mid, tmp = {}, base                                # behind the results: the stretched signals that still await their rate conversion
        for i, pl in enumerate(plans):
            if pl is not None and pl.p != pl.q and pl.p_r != pl.q_r:
                mid[i] = tmp
                tmp = -(-(tmp + pl.n_s) // 8) * 8
        new = torch.empty((max(tmp, 8),), dtype=torch.int16, device=self.device)
        stretch, convert = [], {}
        for i, pl in enumerate(plans):
            if pl is None:
                new[new_offs[i]: new_offs[i] + lens[i]].copy_(buf[offs[i]: offs[i] + lens[i]])
                continue
            if pl.p != pl.q:
                stretch.append([offs[i], lens[i], mid.get(i, new_offs[i]), pl.p, pl.q])
            if pl.p_r != pl.q_r:               # from the stretched signal, or straight from the joined one when tempo == pitch ratio
                convert.setdefault((pl.p_r, pl.q_r), []).append((i, pl.p != pl.q))
        if stretch:
            self.pcm_stretch(buf, stretch, out=new)
        for (p_r, q_r), items in sorted(convert.items()):
            for from_new in (True, False):
                rows = [[mid[i] - base if from_new else offs[i], plans[i].n_s if from_new else lens[i], new_offs[i], plans[i].n_f, 0, 0]
                        for i, stretched in items if stretched == from_new and plans[i].n_f > 0]
                if rows:                       # source and destination are separate parts of ``new``
                    self.pcm_resample(new[base:] if from_new else buf, rows, p_r, q_r, out=new[:base])
        return new[:max(base, 8)], new_offs, new_lens

    # ------------------------------------------------------------------ FLAC output (N15)
    def pcm_flac(self, x: torch.Tensor, rows, sample_rate: int, lpc_order: int = 0):
        """FLAC frames of R final signals in one call (vv_pcm_flac), byte for byte core.audio_processor.flac_encode_frames.
        lpc_order 1 ... 12: with LPC subframes (vv_pcm_flac_lpc; N16), byte for byte the mirror with that order; 0 = vv_pcm_flac as ever.
        x int16 flat on the device; rows = HOST rows (src_off, n, frame0, last): x[src_off, +n) becomes ceil(n / 4096) frames numbered from
        frame0; last = 0 = a block of a stream (n a multiple of 4096).  -> (y, info): y the uint8 device buffer with the frames of all rows
        back to back, info the (R + 1) x 3 int64 device tensor {offset of the row's first frame, smallest frame, largest frame} with
        info[R][0] = the total bytes.  The rows are validated here; the call never synchronises."""
        from .core.audio_processor import FLAC_BLOCK, FLAC_MAX_RATE, check_flac_lpc_order, flac_frame_bound
        assert x.is_cuda and x.dtype == torch.int16 and x.is_contiguous() and x.dim() == 1
        lpc_order = check_flac_lpc_order(lpc_order)
        rows = [[int(v) for v in r] for r in rows]
        if not rows or any(len(r) != 4 for r in rows) or len(rows) > 65535:
            raise ValueError("pcm_flac: 1 to 65535 rows of 4 entries {src_off, n, frame0, last}")
        if isinstance(sample_rate, bool) or int(sample_rate) != sample_rate or not 1 <= int(sample_rate) <= FLAC_MAX_RATE:
            raise ValueError(f"pcm_flac: a sample rate in 1 ... {FLAC_MAX_RATE} Hz is needed")
        n_x, n_y, frames = x.numel(), 0, 0
        for so, n, f0, last in rows:
            nf = -(-n // FLAC_BLOCK)
            if so < 0 or n < 1 or so + n > n_x or f0 < 0 or f0 + nf > 1 << 31 or last not in (0, 1) or (not last and n % FLAC_BLOCK):
                raise ValueError(f"pcm_flac: row {[so, n, f0, last]} does not fit the {n_x} samples of x, the frame numbers below 2^31 or "
                                 f"whole frames of {FLAC_BLOCK} samples where last = 0")
            n_y += (nf - 1) * flac_frame_bound(FLAC_BLOCK) + flac_frame_bound(n - (nf - 1) * FLAC_BLOCK)
            frames += nf
        R = len(rows)
        rows_h = torch.tensor(rows, dtype=torch.int64).reshape(-1, 4)
        rows_d = rows_h.to(self.device)
        y = torch.empty((n_y,), dtype=torch.uint8, device=self.device)
        info = torch.empty((R + 1, 3), dtype=torch.int64, device=self.device)
        ws_bytes = self.lib.vv_pcm_flac_lpc_ws_bytes(frames, R, lpc_order) if lpc_order else self.lib.vv_pcm_flac_ws_bytes(frames, R)
        ws = torch.empty((int(ws_bytes) // 8 + 1,), dtype=torch.int64, device=self.device)
        with self._lock, torch.cuda.device(self.device):
            if lpc_order:
                self._check(self.lib.vv_pcm_flac_lpc(self.ctx, x.data_ptr(), n_x, rows_d.data_ptr(), rows_h.data_ptr(), R, int(sample_rate), lpc_order,
                                                     y.data_ptr(), n_y, info.data_ptr(), ws.data_ptr(), ws.numel() * 8, self._stream()))
            else:
                self._check(self.lib.vv_pcm_flac(self.ctx, x.data_ptr(), n_x, rows_d.data_ptr(), rows_h.data_ptr(), R, int(sample_rate), y.data_ptr(), n_y,
                                                 info.data_ptr(), ws.data_ptr(), ws.numel() * 8, self._stream()))
        return y, info

    # ------------------------------------------------------------------ FLAC input (N17)
    @staticmethod
    def _flac_rows(rows, n_bytes: int, name: str):
        from .core.audio_processor import FLAC_MAX_CLIP
        rows = [[int(v) for v in r] for r in rows]
        if not rows or any(len(r) != 8 for r in rows) or len(rows) > 65535:
            raise ValueError(f"{name}: 1 to 65535 rows of 8 entries {{byte offset, n_bytes, channels, bits, min block, max block, rate, total}}")
        at = 0
        for r in rows:
            off, n, ch, bits, lo, hi, rate, total = r
            if (off < at or off % 4 or n < 0 or off + n + 8 > n_bytes or not 1 <= ch <= 8 or bits not in (8, 16, 24) or not 16 <= hi <= 65535
                    or not 0 <= lo <= hi or not 1 <= rate <= 1048575 or not 0 <= total <= FLAC_MAX_CLIP):
                raise ValueError(f"{name}: row {r} does not fit the {n_bytes} bytes of data (ascending, 4-byte aligned, 8 bytes of padding behind "
                                 f"the last clip) or the decoder's limits")
            at = off + n
        return rows

    def flac_index(self, data: torch.Tensor, rows):
        """vv_flac_index: the frames of R FLAC clips whose frame bytes lie back to back in ``data`` (uint8 on the device,
        each clip 4-byte aligned, 8 bytes of padding behind the last).  rows = HOST rows {byte offset, n_bytes, channels, bits, min block,
        max block, rate, total}.  -> (info R x 4 int64 on the device {status, byte, frames, samples}, the workspace flac_decode consumes).
        The rows are validated here before anything is launched; the call never synchronises."""
        assert data.is_cuda and data.dtype == torch.uint8 and data.is_contiguous() and data.dim() == 1
        n_bytes = data.numel()
        if not 8 <= n_bytes <= (1 << 31) - 64 or data.data_ptr() % 8:
            raise ValueError("flac_index: 8 ... 2^31 - 64 bytes of data, 8-byte aligned")
        rows = self._flac_rows(rows, n_bytes, "flac_index")
        R = len(rows)
        rows_h = torch.tensor(rows, dtype=torch.int64).reshape(-1, 8)
        rows_d = rows_h.to(self.device)
        info = torch.empty((R, 4), dtype=torch.int64, device=self.device)
        ws = torch.empty((int(self.lib.vv_flac_index_ws_bytes(n_bytes, R)) // 8 + 1,), dtype=torch.int64, device=self.device)
        with self._lock, torch.cuda.device(self.device):
            self._check(self.lib.vv_flac_index(self.ctx, data.data_ptr(), n_bytes, rows_d.data_ptr(), rows_h.data_ptr(), R, info.data_ptr(),
                                               ws.data_ptr(), ws.numel() * 8, self._stream()))
        return info, (ws, rows_h, rows_d)

    def flac_decode(self, data: torch.Tensor, index, lay, pcm: torch.Tensor):
        """vv_flac_decode: the clips ``flac_index`` passed, into ``pcm`` (uint8 on the device) as the interleaved little-endian PCM
        vv_ingest_pcm reads.  index = flac_index's second result; lay = HOST rows {pcm byte offset, frames, samples} per clip (a refused
        clip: frames = samples = 0).  -> info2 R x 2 int64 on the device {status, byte}: non-zero where a restored sample left its range."""
        ws, rows_h, rows_d = index
        assert data.is_cuda and data.dtype == torch.uint8 and pcm.is_cuda and pcm.dtype == torch.uint8 and pcm.is_contiguous() and pcm.dim() == 1
        R, n_pcm = rows_h.shape[0], pcm.numel()
        lay = [[int(v) for v in r] for r in lay]
        if len(lay) != R or any(len(r) != 3 for r in lay):
            raise ValueError("flac_decode: one row {pcm byte offset, frames, samples} per clip")
        full, F, S, P, at = [], 0, 0, 0, 0
        for (off, frames, samples), row in zip(lay, rows_h.tolist()):
            nbytes = samples * row[2] * (4 if row[3] == 24 else row[3] // 8)
            if off < at or frames < 0 or samples < frames or off + nbytes > n_pcm:
                raise ValueError(f"flac_decode: row {[off, frames, samples]} does not fit the {n_pcm} bytes of pcm, in ascending order")
            full.append([off, frames, samples, F, P, S])
            at, F, S, P = off + nbytes, F + frames, S + samples, P + samples * row[2]
        lay_h = torch.tensor(full, dtype=torch.int64).reshape(-1, 6)
        lay_d = lay_h.to(self.device)
        info2 = torch.empty((R, 2), dtype=torch.int64, device=self.device)
        ws2 = torch.empty((int(self.lib.vv_flac_decode_ws_bytes(P, F)) // 8 + 1,), dtype=torch.int64, device=self.device)
        with self._lock, torch.cuda.device(self.device):
            self._check(self.lib.vv_flac_decode(self.ctx, data.data_ptr(), data.numel(), rows_d.data_ptr(), rows_h.data_ptr(), R, lay_d.data_ptr(),
                                                lay_h.data_ptr(), ws.data_ptr(), ws.numel() * 8, pcm.data_ptr(), n_pcm, info2.data_ptr(),
                                                ws2.data_ptr(), ws2.numel() * 8, self._stream()))
        return info2

    def flac_clips(self, files, pcm: Optional[torch.Tensor] = None, pcm_offsets=None):
        """Complete FLAC files (bytes) -> their PCM on the device, without a decoded sample crossing the bus: container parsing on the
        host, one upload of the frame bytes, flac_index, ONE small readback of info (32 R bytes, the synchronisation), flac_decode, one
        small readback of info2.  -> (pcm uint8 on the device, [per file: (byte offset, frames, width, rate, channels) or the FlacError
        the mirror would raise]).  A refused file does not disturb the others.  With ``pcm`` / ``pcm_offsets`` None the buffer is laid
        out here (4-byte aligned clips); else ``pcm_offsets(sizes) -> (buffer, offsets)`` lets the caller place the clips in a buffer
        it shares with other PCM."""
        from .core.audio_processor import FlacError, flac_container
        infos, parts, rows, pos = [], [], [], 0
        for data in files:
            data = bytes(data)
            try:
                fi = flac_container(data)
            except FlacError as e:
                infos.append(e)
                continue
            infos.append(fi)
            body = data[fi.start:]
            rows.append([pos, len(body), fi.channels, fi.bits, fi.min_block, fi.max_block, fi.rate, fi.total])
            parts.append(body + b"\0" * (-len(body) % 4))
            pos += len(parts[-1])
        live = [i for i, fi in enumerate(infos) if not isinstance(fi, FlacError)]
        out, sizes, lay = list(infos), [0] * len(files), []
        if live:
            buf = torch.frombuffer(bytearray(b"".join(parts) + b"\0" * (-pos % 8 + 8)), dtype=torch.uint8).to(self.device)
            info_d, index = self.flac_index(buf, rows)
            info = info_d.cpu().tolist()                          # the one synchronisation in front of the layout
            for i, (status, byte, frames, samples), row in zip(live, info, rows):
                if status:
                    out[i] = FlacError(status, infos[i].start + byte)
                    lay.append([0, 0])
                else:
                    sizes[i] = samples * row[2] * (4 if row[3] == 24 else row[3] // 8)
                    lay.append([frames, samples])
        if pcm_offsets is None:
            offs, at = [], 0
            for n in sizes:
                offs.append(at)
                at += n + (-n % 4)
            pcm = torch.empty((max(at, 8),), dtype=torch.uint8, device=self.device)
        else:
            pcm, offs = pcm_offsets(sizes)
        if live:
            at = 0
            for j, i in enumerate(live):                          # a refused clip sits, empty, where the previous one ended
                if lay[j][1]:
                    at = offs[i]
                lay[j] = [at] + lay[j]
                at += sizes[i]
            info2 = self.flac_decode(buf, index, lay, pcm).cpu().tolist()
            for j, i in enumerate(live):
                if isinstance(out[i], FlacError):
                    continue
                if info2[j][0]:
                    out[i] = FlacError(info2[j][0], infos[i].start + info2[j][1])
                else:
                    out[i] = (offs[i], lay[j][2], {8: 1, 16: 2, 24: 4}[rows[j][3]], rows[j][6], rows[j][2])
        return pcm, out

    def _flac_files(self, buf: torch.Tensor, offs, lens, sample_rate: int, lpc_order: int = 0):
        """The last step of finish_output with encoding "flac": one vv_pcm_flac (lpc_order > 0: vv_pcm_flac_lpc) call over the requests, ONE small copy of info (24 (R + 1)
        bytes, the one synchronisation), one copy of exactly info[R][0] bytes; the host puts each request's stream header in front, with
        its true sample count and its frame sizes.  An empty request is a header alone."""
        import numpy as np
        from .core.audio_processor import flac_stream_header
        sel = [i for i, n in enumerate(lens) if n > 0]
        frames = {}
        if sel:
            y, info = self.pcm_flac(buf, [[offs[i], lens[i], 0, 1] for i in sel], sample_rate, lpc_order)
            info = info.cpu().numpy()
            total = int(info[len(sel), 0])
            host = y[:total].cpu().numpy()
            for j, i in enumerate(sel):
                end = int(info[j + 1, 0]) if j + 1 < len(sel) else total
                frames[i] = (host[int(info[j, 0]): end], int(info[j, 1]), int(info[j, 2]))
        out = []
        for i, n in enumerate(lens):
            data, lo, hi = frames.get(i, (np.zeros(0, np.uint8), 0, 0))
            out.append(np.concatenate([np.frombuffer(flac_stream_header(sample_rate, n, lo, hi), np.uint8), data]))
        return out

    def finish_output(self, pcm: torch.Tensor, plans, cross_fade_duration: float, sample_rate: int, rate: Optional[int] = None,
                      encoding: str = "pcm16", loudness=None, peak_dbfs: float = -1.0, limiter=None, pitch=None, tempo=None, flac_lpc_order: int = 0):
        """The whole output stage of R requests on the caller's stream: join (-> pitch and tempo) (-> loudness) (-> limiter) (-> output rate)
        (-> G.711), then ONE device-to-host copy of the final bytes.  pcm int16 on the device, plans = per request its chunks' (src_off, len)
        spans.  pitch (semitones) / tempo = one value for every request, or a per-request list with None entries (N14; all None = nothing
        new is called): core.audio_processor.prosody_plan turns them into a WSOLA stretch and a rate conversion on the joined signal, and
        every later step runs on the result, so levels and the ceiling are those of what is heard.
        loudness = a target in LUFS for every request, or a per-request list with None entries (N12; None = nothing new is called);
        peak_dbfs = its sample-peak ceiling.  limiter = None | "sample" | "true" for every request, or a per-request list (N13; None =
        nothing new is called): a request with a limiter is measured only (pcm_loudness, out="measure") and takes its uncapped loudness
        gain, or the gain 1 without a target, through pcm_limit in place; the others keep the capped gain of N12.
        encoding "flac" (N15): the final PCM goes through pcm_flac instead of the one copy: a small copy of the frames' sizes, then a copy
        of exactly the frames' bytes; each request comes back as a complete FLAC file.  flac_lpc_order 1 ... 12 (N16) adds LPC subframes
        (vv_pcm_flac_lpc instead of vv_pcm_flac) and is refused with another encoding.
        -> a list of R numpy arrays: int16 at ``rate`` (None = sample_rate), uint8 G.711 codes, or the uint8 bytes of a FLAC file."""
        from .core.audio_processor import check_flac_lpc_order, resample_len
        if check_flac_lpc_order(flac_lpc_order) and encoding != "flac":
            raise ValueError("finish_output: flac_lpc_order belongs to the encoding 'flac'")
        buf, offs, lens = self.join_chunks(pcm, plans, cross_fade_duration, sample_rate)
        pitch, tempo = [list(v) if isinstance(v, (list, tuple)) else [v] * len(lens) for v in (pitch, tempo)]
        if len(pitch) != len(lens) or len(tempo) != len(lens):
            raise ValueError("finish_output: one pitch and one tempo entry per request")
        if any(v is not None for v in pitch + tempo):
            buf, offs, lens = self._prosody(buf, offs, lens, pitch, tempo)
        if isinstance(loudness, (list, tuple)):
            if len(loudness) != len(lens):
                raise ValueError("finish_output: one loudness entry per request")
            if all(v is None for v in loudness):
                loudness = None
        if isinstance(limiter, (list, tuple)):
            if len(limiter) != len(lens):
                raise ValueError("finish_output: one limiter entry per request")
            if all(v is None for v in limiter):
                limiter = None
        if limiter is not None:
            from .core.audio_processor import LIMITER_MODES, check_limiter
            lims = [check_limiter(v) for v in (limiter if isinstance(limiter, (list, tuple)) else [limiter] * len(lens))]
            louds = list(loudness) if isinstance(loudness, (list, tuple)) else [loudness] * len(lens)
            plain = [i for i in range(len(lens)) if lims[i] is None and louds[i] is not None]
            if plain:                      # the requests without a limiter: the capped gain of N12, as below
                self.pcm_loudness(buf, [[offs[i], lens[i], offs[i]] for i in plain], sample_rate, [louds[i] for i in plain], peak_dbfs, out=buf)
            for mode in LIMITER_MODES:
                sel = [i for i in range(len(lens)) if lims[i] == mode]
                if not sel:
                    continue
                rows, tg, meas = [[offs[i], lens[i], offs[i]] for i in sel], [louds[i] for i in sel], None
                if any(t is not None for t in tg):
                    _none, meas = self.pcm_loudness(buf, rows, sample_rate, tg, peak_dbfs, out="measure", stats=True)
                self.pcm_limit(buf, rows, sample_rate, peak_dbfs, mode, meas=meas, targets=tg if meas is not None else None, out=buf)
        elif loudness is not None:         # in place on the joined buffer: the apply pass is elementwise
            sel = [i for i in range(len(lens)) if not isinstance(loudness, (list, tuple)) or loudness[i] is not None]
            tg = [loudness[i] for i in sel] if isinstance(loudness, (list, tuple)) else loudness
            self.pcm_loudness(buf, [[offs[i], lens[i], offs[i]] for i in sel], sample_rate, tg, peak_dbfs, out=buf)
        if rate is not None and int(rate) != int(sample_rate):
            _taps, up, down, _skip = self._output_taps(int(sample_rate), int(rate))
            rows, pos = [], 0
            for o, n in zip(offs, lens):
                n_out = resample_len(n, up, down)
                rows.append([o, n, pos, n_out, 0, 0])
                pos += n_out
            buf = self.pcm_resample(buf, rows, sample_rate, rate, n_y=pos) if pos else buf[:0]
            offs, lens = [r[2] for r in rows], [r[3] for r in rows]
        if encoding == "flac":             # N15: variable-length output -- the frames' total comes back first, then exactly that many bytes
            return self._flac_files(buf, offs, lens, int(sample_rate) if rate is None else int(rate), flac_lpc_order)
        if encoding != "pcm16":
            rows, pos = [], 0
            for o, n in zip(offs, lens):
                rows.append([o, n, pos])
                pos += n
            buf = self.pcm_encode(buf, rows, encoding, n_y=pos) if pos else torch.empty((0,), dtype=torch.uint8, device=self.device)
            offs = [r[2] for r in rows]
        host = buf.cpu().numpy()
        return [host[o: o + n] for o, n in zip(offs, lens)]

    def output_stream_backends(self, sample_rate: int, rate: Optional[int], encoding: str, max_upload: int = 1 << 18):
        """(resample, encode) callables for core.audio_processor.OutputStream on this device: host blocks go up in pieces of at most
        ``max_upload`` samples (0.5 MB), through vv_pcm_resample / vv_pcm_encode, and come back.  With encoding "flac" the second one is
        the ``encode(pcm, frame0, last[, lpc_order])`` of core.audio_processor.FlacStream (vv_pcm_flac, vv_pcm_flac_lpc), which sits behind
        the OutputStream."""
        import numpy as np

        def up_(x):
            parts = [torch.from_numpy(np.ascontiguousarray(x[i: i + max_upload])).to(self.device) for i in range(0, x.size, max_upload)]
            return parts[0] if len(parts) == 1 else torch.cat(parts)

        def resample(x, m0, i0, n_out):
            x = np.asarray(x, dtype=np.int16).reshape(-1)
            if n_out <= 0:
                return np.zeros(0, np.int16)
            xd = up_(x) if x.size else torch.zeros((8,), dtype=torch.int16, device=self.device)
            return self.pcm_resample(xd, [[0, x.size, 0, n_out, m0, i0]], sample_rate, rate, n_y=n_out).cpu().numpy()

        def encode(y):
            y = np.asarray(y, dtype=np.int16).reshape(-1)
            if y.size == 0:
                return np.zeros(0, np.uint8)
            return self.pcm_encode(up_(y), [[0, y.size, 0]], encoding, n_y=y.size).cpu().numpy()

        def flac(pcm, frame0, last, lpc_order=0):      # FlacStream's back end (N15, N16): whole blocks (last = False) and the final short frame alike
            pcm = np.asarray(pcm, dtype=np.int16).reshape(-1)
            if pcm.size == 0:
                return np.zeros(0, np.uint8)
            y, info = self.pcm_flac(up_(pcm), [[0, pcm.size, int(frame0), 1 if last else 0]], sample_rate if rate is None else rate, lpc_order)
            return y[: int(info[1, 0])].cpu().numpy()

        return (resample if rate is not None and int(rate) != int(sample_rate) else None), \
            (flac if encoding == "flac" else encode if encoding != "pcm16" else None)

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
        self._host = (C.c_int32 * B)(*self.seq_host)
        nb_t, nb_d = C.c_uint64(), C.c_uint64()
        eng._check(eng.lib.vv_transformer_ws_bytes(eng.ctx, B, N, self._host, C.byref(nb_t)))
        eng._check(eng.lib.vv_decode_ws_bytes(eng.ctx, B, t_gen_max, C.byref(nb_d)))
        self.ws = torch.empty((max(int(nb_t.value), int(nb_d.value)),), dtype=torch.uint8, device=dev)
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
