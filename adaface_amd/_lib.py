"""ctypes binding of libadaface_hip.so (include/adaface_hip.h).

The library is the product: if it is missing or fails to load this module raises —
there is no CPU or eager-PyTorch fallback anywhere in adaface_amd.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

AF_DTYPE_BF16 = 0
AF_DTYPE_F32 = 1
AF_DTYPE_F16 = 2
DTYPES = {"bf16": AF_DTYPE_BF16, "bfloat16": AF_DTYPE_BF16, "f32": AF_DTYPE_F32, "fp32": AF_DTYPE_F32,
          "float32": AF_DTYPE_F32, "f16": AF_DTYPE_F16, "fp16": AF_DTYPE_F16, "float16": AF_DTYPE_F16}

_LIB_PATH = Path(__file__).resolve().parent / "libadaface_hip.so"


class AfConfig(C.Structure):
    """struct af_config (include/adaface_hip.h)."""
    _fields_ = [
        ("dtype", C.c_int),
        ("build_unet", C.c_int),
        ("in_channels", C.c_int), ("model_channels", C.c_int), ("out_channels", C.c_int),
        ("num_res_blocks", C.c_int),
        ("n_attention_resolutions", C.c_int), ("attention_resolutions", C.c_int * 8),
        ("n_channel_mult", C.c_int), ("channel_mult", C.c_int * 8),
        ("num_heads", C.c_int), ("context_dim", C.c_int), ("transformer_depth", C.c_int),
        ("n_context_layers", C.c_int),
        ("build_vae", C.c_int),
        ("vae_ch", C.c_int), ("vae_out_ch", C.c_int), ("vae_num_res_blocks", C.c_int),
        ("vae_z_channels", C.c_int), ("vae_embed_dim", C.c_int),
        ("n_vae_ch_mult", C.c_int), ("vae_ch_mult", C.c_int * 8),
        ("build_vae_encoder", C.c_int), ("vae_in_channels", C.c_int),
        ("build_clip", C.c_int),
        ("clip_vocab", C.c_int), ("clip_hidden", C.c_int), ("clip_layers", C.c_int), ("clip_heads", C.c_int),
        ("clip_intermediate", C.c_int), ("clip_max_pos", C.c_int),
        ("build_controlnet", C.c_int), ("hint_channels", C.c_int),
    ]


class AfError(RuntimeError):
    pass


_lib = None

# every symbol include/adaface_hip.h declares: (name, restype, argtypes)
_P = C.c_void_p
_SIGS = [
    ("af_last_error", C.c_char_p, []),
    ("af_version", C.c_int, []),
    ("af_create", C.c_int, [C.c_int, C.POINTER(AfConfig), C.POINTER(_P)]),
    ("af_destroy", None, [_P]),
    ("af_load_tensor", C.c_int, [_P, C.c_char_p, _P, C.c_int, C.POINTER(C.c_int64)]),
    ("af_load_tensor_device", C.c_int, [_P, C.c_char_p, _P, C.c_int, C.POINTER(C.c_int64)]),
    ("af_load_tensor_lora", C.c_int, [_P, C.c_char_p, _P, C.c_int, C.c_int, C.POINTER(C.c_int64), C.c_int, C.POINTER(_P), C.POINTER(_P),
                                      C.POINTER(C.c_int), C.POINTER(C.c_float)]),
    ("af_op_lora_repack", C.c_int, [C.c_int, _P] + [C.c_int] * 8 + [C.POINTER(_P), C.POINTER(_P), C.POINTER(C.c_int),
                                                                    C.POINTER(C.c_float), _P, _P]),
    ("af_num_tensors", C.c_int, [_P]),
    ("af_tensor_name", C.c_char_p, [_P, C.c_int]),
    ("af_tensor_loaded", C.c_int, [_P, C.c_int]),
    ("af_tensor_shape", C.c_int, [_P, C.c_int, C.POINTER(C.c_int64)]),
    ("af_set_context", C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P]),
    ("af_unet_forward", C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P]),
    ("af_unet_forward_twin", C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P]),
    ("af_unet_forward_cached", C.c_int, [_P, _P, _P, _P] + [C.c_int] * 6 + [_P]),
    ("af_unet_cache_invalidate", C.c_int, [_P]),
    ("af_ddim_step", C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float,
                               C.c_float, _P, _P, _P]),
    ("af_dpmpp_coeffs", C.c_int, [C.c_double, C.c_double, C.c_double, C.POINTER(C.c_double)]),
    ("af_dpmpp_step", C.c_int, [_P, _P, _P, _P, C.c_int64] + [C.c_float] * 7 + [_P, _P, _P]),
    ("af_philox4x32_10", C.c_int, [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    ("af_philox_randn", C.c_int, [_P, C.c_int64, C.c_int64, _P, C.c_int64, C.c_uint64, C.c_uint32, C.c_uint32, _P]),
    ("af_dpmpp_sde_coeffs", C.c_int, [C.c_double, C.c_double, C.c_double, C.POINTER(C.c_double)]),
    ("af_dpmpp_sde_step", C.c_int, [_P, _P, _P, _P, C.c_int64] + [C.c_float] * 7 + [_P, _P, C.c_float, _P, C.c_int64, _P, C.c_int64,
                                    C.c_uint64, C.c_uint32, _P]),
    ("af_noise_blend", C.c_int, [_P, _P, _P, C.c_int, _P, C.c_int64, C.c_int, C.c_int64, C.c_float, C.c_float, _P, C.c_int64,
                                 C.c_uint64, C.c_uint32, C.c_uint32, _P, _P]),
    ("af_noise_blend_launches", C.c_int64, []),
    ("af_lcm_coeffs", C.c_int, [C.c_double, C.c_double, C.c_double, C.c_int64, C.c_double, C.c_double, C.POINTER(C.c_double)]),
    ("af_lcm_step", C.c_int, [_P, _P, _P, C.c_int64] + [C.c_float] * 8 + [_P, _P, _P, C.c_int64, _P, C.c_int64, C.c_uint64,
                              C.c_uint32, _P]),
    ("af_lcm_step_launches", C.c_int64, []),
    ("af_set_regions", C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    ("af_region_state", C.c_int, [_P, C.POINTER(C.c_int)]),
    ("af_region_plan_query", C.c_int, [C.c_int] * 4 + [C.POINTER(C.c_int64)]),
    ("af_region_attn_launches", C.c_int64, []),
    ("af_op_region_weights", C.c_int, [_P] + [C.c_int] * 4 + [_P, _P, _P]),
    ("af_op_region_attention", C.c_int, [C.c_int, _P, _P, _P, _P, _P] + [C.c_int] * 6 + [C.c_float, C.c_int, C.c_int, _P]),
    ("af_sag_taps", C.c_int, [C.c_double, C.POINTER(C.c_double)]),
    ("af_op_sag_mass", C.c_int, [C.c_int, _P, _P, _P, _P] + [C.c_int] * 6 + [_P]),
    ("af_sag_degrade", C.c_int, [_P, _P, _P, _P] + [C.c_int] * 4 + [C.c_float, C.c_float, C.c_double, _P]),
    ("af_sag_set", C.c_int, [_P, C.c_int]),
    ("af_sag_state", C.c_int, [_P, C.POINTER(C.c_int)]),
    ("af_sag_read", C.c_int, [_P, _P, C.c_int64, _P]),
    ("af_sag_mass_launches", C.c_int64, []),
    ("af_sag_degrade_launches", C.c_int64, []),
    ("af_resample_taps", C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    ("af_resample_plan_create", C.c_int, [C.c_int] * 5 + [C.POINTER(_P)]),
    ("af_resample_plan_destroy", C.c_int, [_P]),
    ("af_resample_plan_tables", C.c_int, [_P, C.POINTER(C.c_int), _P, _P, _P, _P]),
    ("af_resample2d", C.c_int, [_P, _P, _P, C.c_int64, _P]),
    ("af_resample2d_launches", C.c_int64, []),
    ("af_lincomb", C.c_int, [_P, C.c_int64, _P, C.c_float, _P, C.c_float, _P, C.c_float, _P, C.c_float, C.c_int, _P]),
    ("af_vae_decode", C.c_int, [_P, _P, C.c_float, _P, _P, C.c_int, C.c_int, C.c_int, _P]),
    ("af_to_uint8", C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P]),
    ("af_arena_bytes", C.c_int64, [_P]),
    ("af_prof_enable", C.c_int, [C.c_int]),
    ("af_prof_reset", C.c_int, []),
    ("af_set_conv_attn", C.c_int, [_P, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("af_vae_encode", C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, _P]),
    ("af_posterior_sample", C.c_int, [_P, _P, C.c_float, _P, C.c_int, C.c_int, C.c_int, _P]),
    ("af_prof_set_stride", C.c_int, [C.c_int]),
    ("af_last_gemm_plan", C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("af_prof_collect", C.c_int, [C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_double),
                                  C.POINTER(C.c_double)]),
    ("af_prof_event_overhead_us", C.c_double, [_P, C.c_int]),
    ("af_unet_num_blocks", C.c_int, [_P]),
    ("af_unet_block_shape", C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("af_unet_set_tap", C.c_int, [_P, C.c_int, _P]),
    ("af_gemm_plan_counts", C.c_int, [C.POINTER(C.c_int64)]),
    ("af_gemm_plan_counts_reset", C.c_int, []),
    ("af_gemm_plan_query", C.c_int, [C.c_int, C.c_int64] + [C.c_int] * 16 + [C.POINTER(C.c_int64)]),
    ("af_norm_plan_query", C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    ("af_attn_plan_query", C.c_int, [C.c_int] * 8 + [C.POINTER(C.c_int64)]),
    ("af_attn_plan_counts", C.c_int, [C.POINTER(C.c_int64)]),
    ("af_knob_set", C.c_int, [C.c_char_p, C.c_int]),
    ("af_knob_get", C.c_int, [C.c_char_p, C.POINTER(C.c_int)]),
    ("af_knob_reset", C.c_int, []),
    ("af_op_conv2d", C.c_int, [C.c_int, _P, _P, _P, _P, _P] + [C.c_int] * 9 + [_P]),
    ("af_op_linear", C.c_int, [C.c_int, _P, _P, _P, _P, _P, C.c_int64, C.c_int, C.c_int, C.c_int, _P]),
    ("af_op_conv2d_ex", C.c_int, [C.c_int, _P, _P, _P, _P, _P, C.c_float, _P] + [C.c_int] * 10 + [_P]),
    ("af_op_linear_ex", C.c_int, [C.c_int, _P, _P, _P, _P, C.c_float, _P, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    ("af_op_groupnorm", C.c_int, [C.c_int, _P, _P, _P, C.c_float, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    ("af_op_conv_gn", C.c_int, [_P, _P, _P, _P, _P, _P, C.c_float, C.c_int, _P, _P] + [C.c_int] * 5 + [_P]),
    ("af_set_fp8", C.c_int, [_P, C.c_int]),
    ("af_fp8_gemm_launches", C.c_int64, []),
    ("af_set_fp8_scope", C.c_int, [_P, C.c_int]),
    ("af_get_fp8_scope", C.c_int, [_P]),
    ("af_ff8_launches", C.c_int64, []),
    ("af_op_ff_fp8", C.c_int, [_P] * 4 + [C.c_float] + [_P] * 5 + [C.c_int64] + [C.c_int] * 5 + [_P, _P, _P, C.POINTER(C.c_int), _P]),
    ("af_fp8_num_sites", C.c_int, [_P]),
    ("af_fp8_site_name", C.c_char_p, [_P, C.c_int]),
    ("af_fp8_record", C.c_int, [_P, C.c_int, _P]),
    ("af_fp8_read_record", C.c_int, [_P, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_int64), _P]),
    ("af_fp8_get_shifts", C.c_int, [_P, C.c_int, C.POINTER(C.c_int)]),
    ("af_fp8_set_shifts", C.c_int, [_P, C.c_int, C.POINTER(C.c_int)]),
    ("af_fp8_shift_for_amax", C.c_int, [C.c_float, C.c_int]),
    ("af_halo8_launches", C.c_int64, []),
    ("af_rowpanel_launches", C.c_int64, []),
    ("af_up_phase4_launches", C.c_int64, []),
    ("af_gn_producer_launches", C.c_int64, []),
    ("af_attn_short_launches", C.c_int64, []),
    ("af_gn_consumer_launches", C.c_int64, []),
    ("af_xattn_fused_launches", C.c_int64, []),
    ("af_conv_attn_short_launches", C.c_int64, []),
    ("af_op_conv_attention", C.c_int, [C.c_int, _P, _P, _P, _P] + [C.c_int] * 6 + [C.c_float] + [C.c_int] * 3 + [_P]),
    ("af_op_vae_attention", C.c_int, [C.c_int, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, C.POINTER(C.c_int), _P]),
    ("af_op_xattn_fused", C.c_int, [C.c_void_p] * 10 + [C.c_int] * 3 + [C.c_void_p]),
    ("af_op_conv2d_fp8", C.c_int, [_P, _P, _P, _P, _P] + [C.c_int] * 10 + [_P]),
    ("af_op_groupnorm_fp8", C.c_int, [_P, _P, _P, C.c_float, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    ("af_op_layernorm_fp8", C.c_int, [_P, _P, _P, C.c_float, _P, C.c_int64, C.c_int, C.c_int, _P]),
    ("af_op_groupnorm_fp8_rec", C.c_int, [_P, _P, _P, C.c_float, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    ("af_op_layernorm_fp8_rec", C.c_int, [_P, _P, _P, C.c_float, _P, C.c_int64, C.c_int, C.c_int, _P, _P]),
    ("af_op_layernorm", C.c_int, [C.c_int, _P, _P, _P, C.c_float, _P, C.c_int64, C.c_int, _P]),
    ("af_op_attention", C.c_int, [C.c_int, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, _P]),
    ("af_op_attention_ex", C.c_int, [C.c_int, _P, _P, _P, _P, _P] + [C.c_int] * 5 + [C.c_float] + [C.c_int] * 6 + [_P]),
    ("af_clip_embed_tokens", C.c_int, [_P, _P, C.c_int64, _P, _P]),
    ("af_clip_text_forward", C.c_int, [_P, _P, C.c_int, C.c_int, C.c_float, C.c_float, _P, _P]),
    ("af_clip_text_forward3", C.c_int, [_P, _P, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, _P, _P]),
    ("af_op_timestep_embedding", C.c_int, [C.c_int, _P, _P, C.c_int, C.c_int, _P]),
    ("af_op_gn_conv1x1", C.c_int, [_P, _P, _P, C.c_float, _P, _P, _P, _P] + [C.c_int] * 5 + [_P]),
    ("af_op_ln_chain", C.c_int, [C.c_int] + [_P] * 6 + [C.c_float, _P, _P, C.c_int64] + [C.c_int] * 7 + [_P] * 8 +
                                [C.POINTER(C.c_int), _P]),
    ("af_set_tome", C.c_int, [_P, C.c_double, C.c_int]),
    ("af_tome_plan_query", C.c_int, [C.c_int, C.c_int, C.c_double, C.POINTER(C.c_int64)]),
    ("af_tome_num_sites", C.c_int, [_P]),
    ("af_tome_set_tap", C.c_int, [_P, C.c_int, _P]),
    ("af_op_tome_match", C.c_int, [C.c_int, _P] + [C.c_int] * 4 + [C.c_double, C.c_int, _P, _P, _P, _P]),
    ("af_op_tome_merge", C.c_int, [C.c_int, _P, _P, _P, C.c_float, _P] + [C.c_int] * 4 + [_P, _P]),
    ("af_op_tome_unmerge_add", C.c_int, [C.c_int, _P, _P, _P] + [C.c_int] * 4 + [_P, _P]),
    ("af_set_freeu", C.c_int, [_P, C.c_int] + [C.c_double] * 4),
    ("af_freeu_num_sites", C.c_int, [_P]),
    ("af_freeu_site", C.c_int, [_P, C.c_int, C.POINTER(C.c_int)]),
    ("af_freeu_plan_query", C.c_int, [C.c_int] * 6 + [C.POINTER(C.c_int64)]),
    ("af_op_freeu", C.c_int, [C.c_int, _P, _P] + [C.c_int] * 6 + [C.c_double, C.c_double, _P, _P, _P]),
    ("af_set_pag", C.c_int, [_P, C.POINTER(C.c_int), C.c_int]),
    ("af_pag_num_sites", C.c_int, [_P]),
    ("af_pag_site", C.c_int, [_P, C.c_int, C.POINTER(C.c_int)]),
    ("af_pag_plan_query", C.c_int, [_P, C.c_int, C.POINTER(C.c_int)]),
    ("af_unet_forward_pag", C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P]),
    ("af_tgate_set", C.c_int, [_P, C.c_int]),
    ("af_tgate_num_sites", C.c_int, [_P]),
    ("af_tgate_state", C.c_int, [_P, C.POINTER(C.c_int)]),
    ("af_tgate_read_site", C.c_int, [_P, C.c_int, _P, _P]),
    ("af_op_tgate_add", C.c_int, [C.c_int, _P, _P, _P, _P, _P] + [C.c_int] * 9 + [_P]),
    ("af_control_set_hint", C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P]),
    ("af_control_num_residuals", C.c_int, [_P]),
    ("af_control_forward", C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    ("af_unet_set_control", C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int]),
    ("af_control_plan_query", C.c_int, [C.POINTER(AfConfig), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int)]),
    ("af_control_stats", C.c_int, [_P, C.POINTER(C.c_int)]),
    ("af_control_add_launches", C.c_int64, []),
    ("af_op_control_add", C.c_int, [C.c_int, C.c_int, C.POINTER(_P), C.POINTER(_P), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                    C.POINTER(C.c_int64), C.POINTER(C.c_float), C.c_int, C.c_int, _P]),
    ("af_guidance", C.c_int, [_P, _P, _P, C.c_int64, C.c_int64, C.c_float, C.c_float, C.c_float, _P, _P, _P]),
    ("af_guidance_plan_query", C.c_int, [C.c_int64, C.c_int64, C.c_int, C.POINTER(C.c_int64)]),
    ("af_flops_issued", C.c_double, [C.c_int]),
    ("af_clock_probe", C.c_int, [_P, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
]
EXPORTED_SYMBOLS = [s[0] for s in _SIGS]

# AF_LORA_MAX_ADAPTERS / AF_LORA_MAX_RANK (include/adaface_hip.h)
LORA_MAX_ADAPTERS = 8
LORA_MAX_RANK = 256
# the `mode` argument of af_unet_forward_cached (include/adaface_hip.h)
DEEPCACHE_MODES = {"refresh": 1, "reuse": 2}
# ... and its `twin` argument, the form of the forward (AF_UNET_FORM_*); False / True keep their meaning
UNET_FORMS = {False: 0, True: 1, "plain": 0, "twin": 1, "pag": 2}
UNET_FORM_LEGS = {0: 1, 1: 2, 2: 3}
# the mode of af_tgate_set (AF_TGATE_*)
TGATE_MODES = {None: 0, "capture": 1, "replay": 2}
# AF_CONTROL_MAX_SEGMENTS (csrc/af_kernels.h): segments of one ControlNet residual add launch
CONTROL_MAX_SEGMENTS = 16


def lib_path() -> Path:
    return _LIB_PATH


def load():
    """Load the shared library (once) and declare every entry point's signature."""
    global _lib
    if _lib is not None:
        return _lib
    if not _LIB_PATH.exists():
        raise AfError(
            f"{_LIB_PATH} not found: build it with `python -m adaface_amd.build` (needs hipcc). "
            "adaface_amd has no fallback path.")
    lib = C.CDLL(os.fspath(_LIB_PATH))
    for name, res, args in _SIGS:
        fn = getattr(lib, name)  # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def set_knob(name: str, value: int) -> None:
    """af_knob_set: force a planner choice / kernel variant (tests, lab scripts)."""
    check(load().af_knob_set(name.encode(), int(value)), f"af_knob_set({name})")


def reset_knobs() -> None:
    load().af_knob_reset()


def plan_counts(reset: bool = False) -> dict:
    """The launch counters since the last reset.  Conv / linear launches, read off the plan's kernel (AfPlanCount, af_kernels.h):
    tile0..tile5 by the plan's tile (row-panel and 128 x 160 GEMM launches under the tile of the tiled kernel they replace),
    halo (four-wave LDS-halo, not under a tile), splitk (launches that ran more than one K slice), ln_consumer / ln_producer,
    fp8 and up_phase4 (neither under a tile), ff8, halo8 (also under tile5), rowpanel (row-panel and 128 x 160 GEMM launches),
    gn_producer / gn_consumer.  Attention, by the kernel af_launch_attention's plan named (ATTN_KERNELS, AfAttnKernel): attn_flash,
    attn_w4, attn_ring40, attn_ring80, attn_short; the kernels with launchers of their own: xattn_fused, conv_attn_short (neither
    is counted under the five before).  reset=True zeroes all of them."""
    lib = load()
    c = (C.c_int64 * 10)()
    check(lib.af_gemm_plan_counts(c), "af_gemm_plan_counts")
    out = {f"tile{i}": int(c[i]) for i in range(6)}
    out["halo"], out["splitk"], out["ln_consumer"], out["ln_producer"] = int(c[6]), int(c[7]), int(c[8]), int(c[9])
    out["fp8"] = int(lib.af_fp8_gemm_launches())
    out["ff8"] = int(lib.af_ff8_launches())
    out["halo8"] = int(lib.af_halo8_launches())
    out["rowpanel"] = int(lib.af_rowpanel_launches())
    out["up_phase4"] = int(lib.af_up_phase4_launches())
    out["gn_producer"] = int(lib.af_gn_producer_launches())
    a = (C.c_int64 * len(ATTN_KERNELS))()
    check(lib.af_attn_plan_counts(a), "af_attn_plan_counts")
    for i, name in enumerate(ATTN_KERNELS[1:], 1):
        out["attn_" + name] = int(a[i])
    out["gn_consumer"] = int(lib.af_gn_consumer_launches())
    out["xattn_fused"] = int(lib.af_xattn_fused_launches())
    out["conv_attn_short"] = int(lib.af_conv_attn_short_launches())
    if reset:
        lib.af_gemm_plan_counts_reset()
    return out


def gemm_plan_query(dtype, M, N, K, cin_pad, ks=1, stride=1, pad=0, up=0, Hs=1, Ws=None, Ho=1, Wo=None, ldc=None, ldo=None,
                    gn_hw=0, gn_cpg=0, flags=0) -> tuple:
    """af_gemm_plan_query: (kernel, row-panel kind, tile, splitk, halo_tw, group_m, ws_bytes) of the launch these integers
    describe (flags: the AF_PQ_* bits of include/adaface_hip.h).  Host only: no GPU is needed.  A linear is ks = 1 on a 1 x M map."""
    Ws = M if Ws is None else Ws
    Wo = M if Wo is None else Wo
    out = (C.c_int64 * 7)()
    check(load().af_gemm_plan_query(int(dtype), int(M), N, K, cin_pad, ks, stride, pad, up, Hs, Ws, Ho, Wo,
                                    cin_pad if ldc is None else ldc, N if ldo is None else ldo, gn_hw, gn_cpg, flags, out),
          "af_gemm_plan_query")
    return tuple(int(v) for v in out)


def tome_plan_query(H, W, ratio) -> tuple:
    """af_tome_plan_query: (Nd, Ns, r, N') of token merging on an H x W map at `ratio`.  Host only: no GPU is needed."""
    out = (C.c_int64 * 4)()
    check(load().af_tome_plan_query(int(H), int(W), float(ratio), out), "af_tome_plan_query")
    return tuple(int(v) for v in out)


def fill_unet_config(cfg: AfConfig, unet: dict) -> AfConfig:
    """The U-Net fields of af_config from UNetModel constructor arguments (Engine and control_plan_query share it)."""
    ar, cm = list(unet["attention_resolutions"]), list(unet["channel_mult"])
    if len(ar) > 8 or len(cm) > 8:
        raise ValueError("at most 8 entries supported")
    cfg.in_channels = unet["in_channels"]
    cfg.model_channels = unet["model_channels"]
    cfg.out_channels = unet.get("out_channels", unet["in_channels"])
    cfg.num_res_blocks = unet["num_res_blocks"]
    cfg.n_attention_resolutions = len(ar)
    for i, v in enumerate(ar):
        cfg.attention_resolutions[i] = int(v)
    cfg.n_channel_mult = len(cm)
    for i, v in enumerate(cm):
        cfg.channel_mult[i] = int(v)
    cfg.num_heads = unet["num_heads"]
    cfg.context_dim = unet["context_dim"]
    cfg.transformer_depth = unet.get("transformer_depth", 1)
    cfg.n_context_layers = unet.get("n_context_layers", 16)
    return cfg


def control_plan_query(unet: dict, H: int, W: int) -> list:
    """af_control_plan_query: [(C, H, W, element offset for one sample)] of the ControlNet residuals of an H x W latent, in block
    order (input blocks, then the middle block), from the constructor arguments alone.  Host only: no GPU is needed."""
    cfg = fill_unet_config(AfConfig(), unet)
    out = (C.c_int64 * (4 * 64))()
    n = C.c_int()
    check(load().af_control_plan_query(C.byref(cfg), int(H), int(W), 64, out, C.byref(n)), "af_control_plan_query")
    return [tuple(int(out[4 * i + k]) for k in range(4)) for i in range(n.value)]


def control_add_launches() -> int:
    """Launches of the ControlNet residual add kernel since the library was loaded (not part of plan_counts)."""
    return int(load().af_control_add_launches())


def noise_blend_launches() -> int:
    """Launches of the noising + inpainting blend kernel since the library was loaded (not part of plan_counts)."""
    return int(load().af_noise_blend_launches())


FREEU_KERNELS = ("refused", "single", "chunked")           # AfFreeuKernel (csrc/af_kernels.h)


def freeu_plan_query(dtype, H, W, Ch, Cs, version=1) -> dict:
    """af_freeu_plan_query: how FreeU runs on one site's H x W map with Ch backbone and Cs skip channels -- kernel form by name,
    launches (backbone and skip both live), 256-pixel chunks and partial-sum bytes per sample.  Host only: no GPU is needed."""
    out = (C.c_int64 * 4)()
    dt = DTYPES[dtype] if isinstance(dtype, str) else int(dtype)
    check(load().af_freeu_plan_query(dt, int(H), int(W), int(Ch), int(Cs), int(version), out), "af_freeu_plan_query")
    return {"kernel": FREEU_KERNELS[int(out[0])], "launches": int(out[1]), "chunks": int(out[2]), "partial_bytes": int(out[3])}


GUIDANCE_KERNELS = ("refused", "combine", "single", "chunked")   # AfGuidanceKernel (csrc/af_kernels.h)


def guidance_plan_query(n_samples, per_sample, rescale_on) -> dict:
    """af_guidance_plan_query: how af_guidance runs -- kernel form by name, launches, 256-element chunks per sample and
    partial bytes per sample.  Host only: no GPU is needed."""
    out = (C.c_int64 * 4)()
    check(load().af_guidance_plan_query(int(n_samples), int(per_sample), int(bool(rescale_on)), out), "af_guidance_plan_query")
    return {"kernel": GUIDANCE_KERNELS[int(out[0])], "launches": int(out[1]), "chunks": int(out[2]), "partial_bytes": int(out[3])}


GN_KERNELS = ("refused", "small", "fold", "finalize")     # AfGnKernel (csrc/af_kernels.h)
LN_KERNELS = ("refused", "wave_row", "rowgroup")          # AfLnKernel
_Out5 = C.c_int64 * 5


def norm_plan_query(kind, dtype, B=1, HW=None, C=None, pre_npart=0, rows=None) -> dict:
    """af_norm_plan_query: the plan of a norm launch, by name.  Host only: no GPU is needed.
    kind "groupnorm" (B, HW, C[, pre_npart]): {"kernel": one of GN_KERNELS, "P", "nchunk", "npart", "wide"};
    kind "layernorm" (rows, C): {"kernel": one of LN_KERNELS, "nv", "rows_per_block"}.  dtype: a name or an AF_DTYPE_* value."""
    dt = DTYPES[dtype] if isinstance(dtype, str) else int(dtype)
    out = _Out5()   # (the parameter C hides the ctypes module here)
    if kind == "groupnorm":
        check(load().af_norm_plan_query(0, dt, int(B), int(HW), int(C), int(pre_npart), out), "af_norm_plan_query")
        return {"kernel": GN_KERNELS[out[0]], "P": int(out[1]), "nchunk": int(out[2]), "npart": int(out[3]), "wide": bool(out[4])}
    if kind == "layernorm":
        check(load().af_norm_plan_query(1, dt, 1, int(rows), int(C), 0, out), "af_norm_plan_query")
        return {"kernel": LN_KERNELS[out[0]], "nv": int(out[1]), "rows_per_block": int(out[2])}
    raise ValueError(f"norm_plan_query: kind {kind!r}")


ATTN_KERNELS = ("refused", "flash", "w4", "ring40", "ring80", "short")   # AfAttnKernel (csrc/af_kernels.h)


def attn_plan_query(dtype, dh, Nk, ldq, ldk=None, ldv=None, ldo=None, causal=False, lse=False, vt_pack=False) -> dict:
    """af_attn_plan_query: the kernel an attention launch with this head dim, key count, row pitches (elements; ldk, ldv and
    ldo default to ldq) and flags reaches, {"kernel": one of ATTN_KERNELS}.  Honours the knobs attn_ring and attn_short.  Host
    only: no GPU is needed.  dtype: a name or an AF_DTYPE_* value."""
    dt = DTYPES[dtype] if isinstance(dtype, str) else int(dtype)
    ldk = ldq if ldk is None else ldk
    flags = (1 if causal else 0) | (2 if lse else 0) | (4 if vt_pack else 0)
    out = C.c_int64()
    check(load().af_attn_plan_query(dt, int(dh), int(Nk), int(ldq), int(ldk), int(ldk if ldv is None else ldv),
                                    int(ldq if ldo is None else ldo), flags, C.byref(out)), "af_attn_plan_query")
    return {"kernel": ATTN_KERNELS[out.value]}


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = load().af_last_error().decode("utf-8", "replace")
        raise AfError(f"{what or 'libadaface_hip'} failed (rc={rc}): {msg}")


def stream_ptr():
    """Current torch HIP stream as a void* for the C ABI."""
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    """Device/host data pointer of a tensor (None -> NULL)."""
    return C.c_void_p(0 if t is None else t.data_ptr())
