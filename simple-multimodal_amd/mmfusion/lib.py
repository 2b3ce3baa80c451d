"""ctypes binding of ``libmmfusion.so`` (C ABI: ``include/mmfusion.h``).

The library is the product: there is no CPU or eager fallback.  ``load()`` raises if the shared
object is missing, and every wrapper raises ``RuntimeError(mmf_last_error())`` on a negative
return code.  Wrappers take raw device pointers (``tensor.data_ptr()``) and enqueue on the HIP
stream that torch currently uses, so launches are ordered with torch's own work and can be
captured by ``torch.cuda.graph``.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Sequence

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MMF_LIB_PATH") or os.path.join(_HERE, "libmmfusion.so")     # MMF_LIB_PATH: A/B of two builds in one gpurun call

GEMM_NT, GEMM_NN, GEMM_TN = 0, 1, 2
EPI_BIAS, EPI_RELU, EPI_MASK_AUX, EPI_ADD_AUX, EPI_ACCUM, EPI_COLSUM_A, EPI_DROPOUT = 1, 2, 4, 8, 16, 32, 64
EPI_RELU_BITS, EPI_MASK_BITS = 128, 256      # the ReLU / dropout keep-mask as bits: written by the forward, read by the dgrad (aux = the bit buffer)
GEMM_MAX_PROBLEMS, ATTN_MAX_PROBLEMS, LN_MAX_PROBLEMS, COLSUM_MAX_PROBLEMS = 48, 12, 8, 24
LN2_ADD3_MAX_PROBLEMS = 4
EVAL_MAX_HEADS, EVAL_NSUMS = 4, 4

# every symbol include/mmfusion.h declares (tests check the .so exports all of them)
SYMBOLS = (
    "mmf_version", "mmf_last_error", "mmf_device_cu_count", "mmf_gemm_grouped", "mmf_gemm_grouped_ex", "mmf_gemm_relu_bits_bytes", "mmf_gemm_relu_bits_available", "mmf_gemm_select_impl", "mmf_gemm_last_impl", "mmf_gemm_set_persistent_workgroups",
    "mmf_gemm7_set_tile_n", "mmf_gemm7_last_tile_n", "mmf_gemm7_tile_n",
    "mmf_gemm_grouped_chain", "mmf_gemm_chain_available", "mmf_gemm7_chain_tile_n",
    "mmf_attn_fwd_grouped_ex", "mmf_attn_bwd_grouped_ex", "mmf_dropout", "mmf_attn_select_impl",
    "mmf_attn_fwd_grouped", "mmf_attn_bwd_grouped", "mmf_attn_delta_f32", "mmf_attn_bwd_grouped_delta", "mmf_layernorm_fwd_grouped",
    "mmf_layernorm_bwd_grouped", "mmf_layernorm_bwd_add_grouped", "mmf_layernorm_bwd_workspace_bytes", "mmf_layernorm_last_form", "mmf_layernorm2_add3_available", "mmf_layernorm2_add3_fwd_grouped", "mmf_cast_f32_to_bf16", "mmf_cast_bf16_to_f32", "mmf_cast_bf16_to_f32_scaled", "mmf_cast_f32_to_bf16_2d", "mmf_add3_bf16", "mmf_add3_grouped", "mmf_addn_bf16", "mmf_addn_grouped",
    "mmf_meanpool_fwd", "mmf_meanpool_bwd", "mmf_meanpool_cat_fwd", "mmf_meanpool_cat_bwd", "mmf_colsum_bf16", "mmf_colsum_grouped", "mmf_relu_bwd_bf16", "mmf_relu_bwd_mixed",
    "mmf_sqnorm_f32", "mmf_adamw_step", "mmf_adamw_advance", "mmf_skinny_linear_fwd", "mmf_skinny_linear_dgrad", "mmf_skinny_linear_fwd_ex", "mmf_skinny_linear_dgrad_ex", "mmf_skinny_last_strip",
    "mmf_gat3_dense_fwd", "mmf_gat3_dense_bwd", "mmf_infonce_fwd", "mmf_infonce_bwd", "mmf_adaptive_combine_fwd",
    "mmf_adaptive_combine_bwd", "mmf_adaptive_attn_weights", "mmf_linear_narrow_fwd", "mmf_linear_narrow_bwd", "mmf_stack3_embed_fwd",
    "mmf_stack3_embed_bwd", "mmf_rowmask_apply", "mmf_zero_ranges_f32", "mmf_sum_slabs_f32", "mmf_fusion_loss", "mmf_modality_dropout",
    "mmf_attn_weights_mean", "mmf_gemm_f32_grouped", "mmf_gemm_f32_batched", "mmf_softmax_rows_f32", "mmf_softmax_bwd_rows_f32",
    "mmf_layernorm_f32_fwd", "mmf_layernorm_f32_bwd", "mmf_bilstm_workspace_bytes", "mmf_bilstm_layer_fwd", "mmf_bilstm_layer_bwd", "mmf_swap01",
    "mmf_distill_kl", "mmf_fusion_loss_kd", "mmf_robust_head_fwd", "mmf_robust_head_bwd",
    "mmf_fewshot_proto_fwd", "mmf_fewshot_proto_bwd", "mmf_fewshot_dist_fwd", "mmf_fewshot_dist_bwd",
    "mmf_eval_accumulate",
    "mmf_vit_patchify", "mmf_vit_embed_tokens", "mmf_vit_embed_tokens_bwd", "mmf_vit_cls_attn_bwd", "mmf_bias_gelu_bf16", "mmf_bias_gelu_bf16_to", "mmf_bias_gelu_bwd_bf16",
    "mmf_w2v_conv0_stats", "mmf_w2v_conv0_norm_gelu", "mmf_w2v_gelu_window", "mmf_w2v_posconv",
    "mmf_w2v_posconv_bwd_act", "mmf_w2v_posconv_dgrad", "mmf_w2v_posconv_wgrad", "mmf_w2v_weightnorm_bwd",
    "mmf_w2v_window_fold_gelu_bwd", "mmf_w2v_conv0_bwd_stats", "mmf_w2v_conv0_bwd_wgrad",
    "mmf_w2v_conv0_ln_gelu", "mmf_w2v_ln_gelu_window",
    "mmf_deberta_embed", "mmf_deberta_attn_fwd", "mmf_deberta_attn_fwd_lse", "mmf_deberta_attn_bwd", "mmf_deberta_embed_bwd",
    "mmf_deberta_attn_bwd_pos_workspace_bytes", "mmf_deberta_attn_bwd_pos",
    "mmf_deberta_embed_bwd_params_workspace_bytes", "mmf_deberta_embed_bwd_params", "mmf_embedding_scatter_add_f32",
    "mmf_deberta_attn_fwd_drop", "mmf_deberta_attn_bwd_drop", "mmf_deberta_attn_bwd_pos_drop", "mmf_hidden_dropout",
    "mmf_video_prepare", "mmf_video_prepare_patches", "mmf_audio_resample", "mmf_audio_augment",
    "mmf_attn_fwd_grouped_keyed", "mmf_attn_delta_f32_keyed", "mmf_attn_bwd_grouped_delta_keyed", "mmf_bias_gelu_drop_bf16_to",
    "mmf_bias_gelu_drop_bwd_bf16", "mmf_w2v_mask_spans", "mmf_w2v_mask_drop", "mmf_w2v_mask_embed_grad",
    "mmf_attn_bwd_grouped_uniform_available", "mmf_attn_bwd_grouped_uniform_workspace_bytes", "mmf_attn_bwd_grouped_uniform",
    "mmf_attn_bwd_grouped_pooled",
    "mmf_wavlm_gate", "mmf_attn_fwd_relbias",
    "mmf_bert_embed", "mmf_mask_pack_words", "mmf_mask_pack", "mmf_attn_fwd_keymask",
    "mmf_whisper_logmel_scratch_bytes", "mmf_whisper_logmel", "mmf_whisper_feature_window", "mmf_whisper_gelu_window", "mmf_whisper_stem_out",
)


class GemmProblem(C.Structure):
    _fields_ = [("A", C.c_void_p), ("B", C.c_void_p), ("C", C.c_void_p), ("bias", C.c_void_p),
                ("aux", C.c_void_p), ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32),
                ("lda", C.c_int32), ("ldb", C.c_int32), ("ldc", C.c_int32), ("ldaux", C.c_int32)]


GEMM_CHAIN_MAX_SEGMENTS, GEMM_MAX_CHAINS = 4, 12


class GemmSegment(C.Structure):
    _fields_ = [("A", C.c_void_p), ("B", C.c_void_p), ("K", C.c_int32), ("lda", C.c_int32), ("ldb", C.c_int32),
                ("reserved", C.c_int32)]


class GemmChain(C.Structure):
    _fields_ = [("C", C.c_void_p), ("bias", C.c_void_p), ("aux", C.c_void_p), ("M", C.c_int32), ("N", C.c_int32),
                ("ldc", C.c_int32), ("ldaux", C.c_int32), ("num_segments", C.c_int32), ("reserved", C.c_int32),
                ("seg", GemmSegment * GEMM_CHAIN_MAX_SEGMENTS)]


class AttnProblem(C.Structure):
    _fields_ = [("Q", C.c_void_p), ("K", C.c_void_p), ("V", C.c_void_p), ("O", C.c_void_p),
                ("LSE", C.c_void_p), ("dO", C.c_void_p), ("delta", C.c_void_p), ("dQ", C.c_void_p),
                ("dK", C.c_void_p), ("dV", C.c_void_p), ("B", C.c_int32), ("H", C.c_int32),
                ("Tq", C.c_int32), ("Tk", C.c_int32), ("ldq", C.c_int32), ("ldk", C.c_int32),
                ("ldv", C.c_int32), ("ldo", C.c_int32)]


class LnProblem(C.Structure):
    _fields_ = [("x", C.c_void_p), ("y", C.c_void_p), ("gamma", C.c_void_p), ("beta", C.c_void_p),
                ("mean", C.c_void_p), ("rstd", C.c_void_p), ("dy", C.c_void_p), ("dx", C.c_void_p),
                ("dgamma", C.c_void_p), ("dbeta", C.c_void_p), ("rows", C.c_int32)]


class Ln2Add3Problem(C.Structure):
    _fields_ = [("x", C.c_void_p), ("pre_a", C.c_void_p), ("gamma_a", C.c_void_p), ("beta_a", C.c_void_p),
                ("pre_b", C.c_void_p), ("gamma_b", C.c_void_p), ("beta_b", C.c_void_p), ("e", C.c_void_p),
                ("mean_a", C.c_void_p), ("rstd_a", C.c_void_p), ("mean_b", C.c_void_p), ("rstd_b", C.c_void_p),
                ("rows", C.c_int32)]


class GemmExtra(C.Structure):
    _fields_ = [("alpha", C.c_float), ("dropout_p", C.c_float), ("rng_state", C.c_void_p), ("site", C.c_uint32)]


class SkinnyProblem(C.Structure):
    _fields_ = [("X", C.c_void_p), ("W", C.c_void_p), ("Y", C.c_void_p), ("bias", C.c_void_p), ("aux", C.c_void_p),
                ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("ldx", C.c_int32), ("ldw", C.c_int32),
                ("ldy", C.c_int32), ("ldaux", C.c_int32)]


class SkinnyProblemEx(C.Structure):
    _fields_ = [("p", SkinnyProblem), ("Y2", C.c_void_p), ("gate", C.c_void_p), ("dz", C.c_void_p),
                ("ldy2", C.c_int32), ("ldgate", C.c_int32), ("lddz", C.c_int32), ("reserved", C.c_int32)]


class SkinnyExtra(C.Structure):
    _fields_ = [("x_f32", C.c_int32), ("gate_f32", C.c_int32), ("gate_scale", C.c_float), ("dropout_p", C.c_float),
                ("rng_state", C.c_void_p), ("site", C.c_uint32), ("reserved", C.c_uint32)]


SKINNY_MAX_M, SKINNY_MAX_PROBLEMS = 64, 24
ADD3_MAX = 8
ADDN_MAX = 8
ADDN_GROUP_MAX = 4


class AddNProblem(C.Structure):
    _fields_ = [("x", C.c_void_p * 8), ("y", C.c_void_p), ("numel", C.c_int64), ("n", C.c_int32)]


class Add3Problem(C.Structure):
    _fields_ = [("a", C.c_void_p), ("b", C.c_void_p), ("c", C.c_void_p), ("y", C.c_void_p), ("n", C.c_int64)]

ZERO_MAX_RANGES = 48
POOL_MAX = 4


class Gat3Params(C.Structure):
    _fields_ = [("B", C.c_int32), ("heads", C.c_int32), ("C", C.c_int32), ("relu", C.c_int32),
                ("negative_slope", C.c_float), ("dropout_p", C.c_float), ("rng_state", C.c_void_p), ("site", C.c_uint32)]


class BiLstmArgs(C.Structure):
    _fields_ = [("gx", C.c_void_p), ("w_hh", C.c_void_p * 2), ("b_ih", C.c_void_p * 2), ("b_hh", C.c_void_p * 2),
                ("y", C.c_void_p), ("gates", C.c_void_p), ("cell", C.c_void_p), ("dy", C.c_void_p), ("dgates", C.c_void_p),
                ("T", C.c_int32), ("B", C.c_int32), ("H", C.c_int32)]


class ColsumProblem(C.Structure):
    _fields_ = [("x", C.c_void_p), ("out", C.c_void_p), ("M", C.c_int32), ("N", C.c_int32), ("ldx", C.c_int32)]


_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """Load libmmfusion.so (built by ``__graft_entry__.build()`` / ``make -C csrc``)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: the MI355X fusion path has no fallback. Build it with "
            f"`python -c 'import __graft_entry__ as g; g.build()'` or `make -C simple-multimodal_amd/csrc`.")
    # torch first: its wheel bundles its own libamdhip64; libmmfusion.so must bind to THAT copy (same SONAME), or the
    # process ends up with two HIP runtimes and this library's launches fail with "no ROCm-capable device"
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    lib.mmf_last_error.restype = C.c_char_p
    lib.mmf_version.restype = C.c_int
    vp, i32, i64, f32 = C.c_void_p, C.c_int, C.c_int64, C.c_float
    lib.mmf_gemm_grouped.argtypes = [C.POINTER(GemmProblem), i32, i32, i32, i32, vp]
    lib.mmf_gemm_grouped_ex.argtypes = [C.POINTER(GemmProblem), i32, i32, i32, i32, C.POINTER(GemmExtra), vp]
    lib.mmf_gemm_relu_bits_bytes.argtypes = [i32, i32]
    lib.mmf_gemm_relu_bits_bytes.restype = C.c_size_t
    lib.mmf_gemm_relu_bits_available.argtypes = [C.POINTER(GemmProblem), i32, i32, i32, i32, C.POINTER(GemmExtra)]
    lib.mmf_gemm7_tile_n.argtypes = [C.POINTER(GemmProblem), i32, i32]
    lib.mmf_gemm_grouped_chain.argtypes = [C.POINTER(GemmChain), i32, i32, i32, vp]
    lib.mmf_gemm_chain_available.argtypes = [C.POINTER(GemmChain), i32, i32, i32, vp]
    lib.mmf_gemm7_chain_tile_n.argtypes = [C.POINTER(GemmChain), i32, i32]
    lib.mmf_attn_fwd_grouped_ex.argtypes = [C.POINTER(AttnProblem), i32, i32, f32, f32, vp, C.c_uint32, vp]
    lib.mmf_attn_bwd_grouped_ex.argtypes = [C.POINTER(AttnProblem), i32, i32, f32, f32, vp, C.c_uint32, vp]
    lib.mmf_dropout.argtypes = [vp, vp, i64, i32, f32, vp, C.c_uint32, vp]
    lib.mmf_attn_fwd_grouped.argtypes = [C.POINTER(AttnProblem), i32, i32, f32, vp]
    lib.mmf_attn_select_impl.argtypes = [i32]
    lib.mmf_attn_bwd_grouped.argtypes = [C.POINTER(AttnProblem), i32, i32, f32, vp]
    lib.mmf_attn_delta_f32.argtypes = [C.POINTER(AttnProblem), i32, i32, f32, vp]
    lib.mmf_attn_bwd_grouped_delta.argtypes = [C.POINTER(AttnProblem), i32, i32, f32, vp]
    lib.mmf_attn_bwd_grouped_uniform_available.argtypes = [i32, f32]
    lib.mmf_attn_bwd_grouped_uniform_workspace_bytes.argtypes = [C.POINTER(AttnProblem), i32]
    lib.mmf_attn_bwd_grouped_uniform_workspace_bytes.restype = C.c_size_t
    lib.mmf_attn_bwd_grouped_uniform.argtypes = [C.POINTER(AttnProblem), i32, i32, f32, vp, C.c_size_t, vp]
    lib.mmf_attn_bwd_grouped_pooled.argtypes = [C.POINTER(AttnProblem), i32, i32, f32, C.POINTER(C.c_void_p), i32, vp, C.c_size_t, vp]
    lib.mmf_layernorm_fwd_grouped.argtypes = [C.POINTER(LnProblem), i32, i32, f32, vp]
    lib.mmf_layernorm_bwd_grouped.argtypes = [C.POINTER(LnProblem), i32, i32, vp, C.c_size_t, vp]
    lib.mmf_layernorm_bwd_add_grouped.argtypes = [C.POINTER(LnProblem), i32, i32, vp, C.c_size_t, vp]
    lib.mmf_layernorm_bwd_workspace_bytes.argtypes = [i32]
    lib.mmf_layernorm_bwd_workspace_bytes.restype = C.c_size_t
    lib.mmf_layernorm2_add3_available.argtypes = [C.POINTER(C.c_int32), i32, i32]
    lib.mmf_layernorm2_add3_fwd_grouped.argtypes = [C.POINTER(Ln2Add3Problem), i32, i32, f32, vp]
    lib.mmf_cast_f32_to_bf16.argtypes = [vp, vp, i64, vp]
    lib.mmf_cast_bf16_to_f32.argtypes = [vp, vp, i64, vp]
    lib.mmf_cast_bf16_to_f32_scaled.argtypes = [vp, vp, i64, f32, vp]
    lib.mmf_cast_f32_to_bf16_2d.argtypes = [vp, vp, i32, i32, i32, vp]
    lib.mmf_add3_bf16.argtypes = [vp, vp, vp, vp, i64, vp]
    lib.mmf_add3_grouped.argtypes = [C.POINTER(Add3Problem), i32, vp]
    lib.mmf_addn_bf16.argtypes = [C.POINTER(C.c_void_p), i32, vp, i64, i32, vp]
    lib.mmf_addn_grouped.argtypes = [C.POINTER(AddNProblem), i32, vp]
    lib.mmf_meanpool_fwd.argtypes = [vp, vp, i32, i32, i32, i32, vp]
    lib.mmf_meanpool_bwd.argtypes = [vp, vp, i32, i32, i32, i32, vp]
    lib.mmf_meanpool_cat_fwd.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_int), i32, vp, i32, i32, i32, vp]
    lib.mmf_meanpool_cat_bwd.argtypes = [vp, C.POINTER(C.c_void_p), C.POINTER(C.c_int), i32, i32, i32, i32, vp]
    lib.mmf_colsum_bf16.argtypes = [vp, vp, i32, i32, i32, vp]
    lib.mmf_colsum_grouped.argtypes = [C.POINTER(ColsumProblem), i32, vp]
    lib.mmf_relu_bwd_bf16.argtypes = [vp, vp, vp, i64, vp]
    lib.mmf_relu_bwd_mixed.argtypes = [vp, C.c_int, vp, C.c_int, vp, i64, vp]
    lib.mmf_skinny_linear_fwd.argtypes = [C.POINTER(SkinnyProblem), i32, i32, i32, vp]
    lib.mmf_skinny_linear_dgrad.argtypes = [C.POINTER(SkinnyProblem), i32, i32, f32, i32, vp]
    lib.mmf_fusion_loss.argtypes = [vp, i32, vp, i32, i32, f32, C.POINTER(vp), C.POINTER(f32), i32, vp, vp, vp]
    lib.mmf_modality_dropout.argtypes = [C.POINTER(vp), C.POINTER(vp), vp, i32, i32, f32, vp, C.c_uint32, i32, vp]
    lib.mmf_distill_kl.argtypes = [vp, i32, vp, i32, i32, i32, f32, vp, vp, vp]
    lib.mmf_fusion_loss_kd.argtypes = [vp, i32, vp, i32, i32, f32, C.POINTER(vp), C.POINTER(f32), i32, vp, i32, f32, f32, vp, vp, vp]
    pp = C.POINTER(vp)
    lib.mmf_robust_head_fwd.argtypes = [pp, vp, vp, vp, pp, pp, i32, vp, pp, vp, vp, i32, i32, i32, vp]
    lib.mmf_robust_head_bwd.argtypes = [pp, vp, vp, pp, vp, pp, vp, i32, vp, pp, vp, vp, pp, vp, vp, vp, pp, pp,
                                        i32, i32, i32, vp]
    lib.mmf_fewshot_proto_fwd.argtypes = [pp, vp, vp, i32, i32, i32, vp]
    lib.mmf_fewshot_proto_bwd.argtypes = [vp, vp, vp, i32, i32, i32, vp]
    lib.mmf_fewshot_dist_fwd.argtypes = [pp, vp, vp, vp, vp, i32, i32, i32, vp]
    lib.mmf_fewshot_dist_bwd.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp]
    lib.mmf_eval_accumulate.argtypes = [pp, C.POINTER(C.c_int), i32, vp, i32, i32, f32, vp, vp, vp, vp, vp, i64, i64, vp]
    lib.mmf_skinny_linear_fwd_ex.argtypes = [C.POINTER(SkinnyProblemEx), i32, i32, i32, C.POINTER(SkinnyExtra), vp]
    lib.mmf_skinny_linear_dgrad_ex.argtypes = [C.POINTER(SkinnyProblemEx), i32, i32, f32, i32, C.POINTER(SkinnyExtra), vp]
    lib.mmf_sqnorm_f32.argtypes = [vp, i64, vp, vp]
    P3 = C.c_void_p * 3
    lib.mmf_gat3_dense_fwd.argtypes = [vp] * 8 + [C.POINTER(Gat3Params), vp]
    lib.mmf_gat3_dense_bwd.argtypes = [vp] * 12 + [C.POINTER(Gat3Params), vp]
    lib.mmf_infonce_fwd.argtypes = [P3, P3, vp, vp, vp, i32, i32, f32, vp]
    lib.mmf_infonce_bwd.argtypes = [P3, vp, vp, P3, P3, P3, i32, i32, f32, vp]
    lib.mmf_adaptive_combine_fwd.argtypes = [vp] * 6 + [i32, i32, vp]
    lib.mmf_adaptive_combine_bwd.argtypes = [vp] * 10 + [i32, i32, vp]
    lib.mmf_adaptive_attn_weights.argtypes = [vp, vp, i32, i32, i32, vp]
    lib.mmf_attn_weights_mean.argtypes = [vp, vp, i32, i32, i32, i32, vp]
    lib.mmf_linear_narrow_fwd.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp]
    lib.mmf_linear_narrow_bwd.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, i32, vp]
    lib.mmf_stack3_embed_fwd.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, vp]
    lib.mmf_stack3_embed_bwd.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, vp]
    lib.mmf_rowmask_apply.argtypes = [vp, vp, vp, i32, i32, vp]
    lib.mmf_zero_ranges_f32.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), i32, vp]
    lib.mmf_sum_slabs_f32.argtypes = [vp, vp, i64, i32, i32, vp]
    lib.mmf_adamw_step.argtypes = [vp, vp, vp, vp, vp, i64, vp, vp, vp]
    lib.mmf_adamw_advance.argtypes = [vp, vp, vp, vp]
    lib.mmf_bilstm_workspace_bytes.restype = C.c_size_t
    lib.mmf_bilstm_layer_fwd.argtypes = [C.POINTER(BiLstmArgs), vp, C.c_size_t, vp]
    lib.mmf_bilstm_layer_bwd.argtypes = [C.POINTER(BiLstmArgs), vp, C.c_size_t, vp]
    lib.mmf_swap01.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp]
    lib.mmf_vit_patchify.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp]
    lib.mmf_vit_embed_tokens.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp]
    lib.mmf_vit_embed_tokens_bwd.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp]
    lib.mmf_vit_cls_attn_bwd.argtypes = [vp, vp, vp, i32, i32, i32, i32, f32, vp]
    lib.mmf_bias_gelu_bf16.argtypes = [vp, vp, i64, i32, i32, vp]
    lib.mmf_bias_gelu_bf16_to.argtypes = [vp, vp, vp, i64, i32, i32, vp]
    lib.mmf_bias_gelu_bwd_bf16.argtypes = [vp, vp, vp, vp, i64, i32, i32, vp]
    lib.mmf_w2v_conv0_stats.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]
    lib.mmf_w2v_conv0_norm_gelu.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, f32, vp]
    lib.mmf_w2v_gelu_window.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp]
    lib.mmf_w2v_conv0_ln_gelu.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, f32, vp]
    lib.mmf_w2v_ln_gelu_window.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, f32, vp]
    lib.mmf_w2v_window_fold_gelu_bwd.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, vp]
    lib.mmf_w2v_conv0_bwd_stats.argtypes = [vp] * 10 + [i32] * 7 + [f32, i32, vp]
    lib.mmf_w2v_conv0_bwd_wgrad.argtypes = [vp] * 9 + [i32] * 7 + [f32, i32, vp]
    lib.mmf_w2v_posconv.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]
    lib.mmf_w2v_posconv_bwd_act.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]
    lib.mmf_w2v_posconv_dgrad.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]
    lib.mmf_w2v_posconv_wgrad.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]
    lib.mmf_w2v_weightnorm_bwd.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]
    lib.mmf_deberta_embed.argtypes = [vp, vp, vp, vp, vp, f32, vp, i32, vp, i64, i32, i32, vp]
    lib.mmf_deberta_attn_fwd.argtypes = [vp, vp, vp, i32, vp, vp, i32, vp, i32, i32, i32, i32, i32, f32, vp]
    lib.mmf_deberta_attn_fwd_lse.argtypes = [vp, vp, vp, i32, vp, vp, i32, vp, vp, i32, i32, i32, i32, i32, f32, vp]
    lib.mmf_deberta_attn_bwd.argtypes = [vp, vp, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, f32, vp]
    lib.mmf_deberta_embed_bwd.argtypes = [vp, vp, f32, vp, i32, vp, vp, i64, i32, vp]
    lib.mmf_deberta_attn_bwd_pos_workspace_bytes.argtypes = [i32, i32, i32, i32]
    lib.mmf_deberta_attn_bwd_pos_workspace_bytes.restype = C.c_size_t
    lib.mmf_deberta_attn_bwd_pos.argtypes = [vp, vp, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, f32,
                                             vp, vp, i32, vp, C.c_size_t, vp]
    drop = [f32, vp, C.c_uint32, i64]                                  # p, rng_state, site, item0
    lib.mmf_deberta_attn_fwd_drop.argtypes = [vp, vp, vp, i32, vp, vp, i32, vp, vp, i32, i32, i32, i32, i32, f32] + drop + [vp]
    lib.mmf_deberta_attn_bwd_drop.argtypes = [vp, vp, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, f32] + drop + [vp]
    lib.mmf_deberta_attn_bwd_pos_drop.argtypes = ([vp, vp, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, f32,
                                                   vp, vp, i32, vp, C.c_size_t] + drop + [vp])
    lib.mmf_hidden_dropout.argtypes = [vp, vp, vp, i32, i64, i64] + drop + [vp]
    keyed = [C.POINTER(AttnProblem), i32, i32, f32, f32, vp, C.c_uint32, C.c_uint32, vp]       # .., scale, p, rng_state, site, stream_base
    lib.mmf_attn_fwd_grouped_keyed.argtypes = keyed
    lib.mmf_attn_delta_f32_keyed.argtypes = keyed
    lib.mmf_attn_bwd_grouped_delta_keyed.argtypes = keyed
    lib.mmf_bias_gelu_drop_bf16_to.argtypes = [vp, vp, vp, i64, i32, i32, i64] + drop + [vp]
    lib.mmf_bias_gelu_drop_bwd_bf16.argtypes = [vp, vp, vp, vp, i64, i32, i32, i64] + drop + [vp]
    lib.mmf_w2v_mask_spans.argtypes = [vp, i32, i32, i32, C.c_double, i32, i32, vp, C.c_uint32, i64, vp]
    lib.mmf_w2v_mask_drop.argtypes = [vp, vp, vp, vp, i64, i32, i32, i32, i32] + drop + [vp]
    lib.mmf_w2v_mask_embed_grad.argtypes = [vp, vp, vp, i64, i32, i32, i32, i32, i32, vp]
    lib.mmf_deberta_embed_bwd_params_workspace_bytes.argtypes = [i64, i32]
    lib.mmf_deberta_embed_bwd_params_workspace_bytes.restype = C.c_size_t
    lib.mmf_deberta_embed_bwd_params.argtypes = [vp, vp, vp, i32, vp, f32, vp, i32, vp, vp, i32, vp, vp, vp, C.c_size_t, i64, i32, vp]
    lib.mmf_embedding_scatter_add_f32.argtypes = [vp, vp, i32, vp, vp, i64, i32, i32, vp]
    lib.mmf_video_prepare.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]
    lib.mmf_video_prepare_patches.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]
    lib.mmf_audio_resample.argtypes = [vp, vp, vp, i64, vp, i32, i32, i64, i64, i32, i32, i32, vp]
    lib.mmf_audio_augment.argtypes = [vp, vp, vp, vp, vp, C.c_uint32, i32, i64, vp]
    lib.mmf_wavlm_gate.argtypes = [vp, i32, vp, vp, vp, vp, i32, i32, i32, i32, vp]
    lib.mmf_attn_fwd_relbias.argtypes = [C.POINTER(AttnProblem), i32, f32, vp, vp, vp]
    lib.mmf_bert_embed.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, f32, i32, i64, vp, i64, i32, i32, i32, i32, i32, vp]
    lib.mmf_mask_pack_words.argtypes = [i32]
    lib.mmf_mask_pack.argtypes = [vp, i32, vp, i32, i32, vp]
    lib.mmf_attn_fwd_keymask.argtypes = [C.POINTER(AttnProblem), i32, f32, vp, vp]
    lib.mmf_whisper_logmel_scratch_bytes.argtypes = [i32, i32, i32]
    lib.mmf_whisper_logmel_scratch_bytes.restype = C.c_size_t
    lib.mmf_whisper_logmel.argtypes = [vp, i64, vp, vp, vp, vp, vp, vp, C.c_size_t, i32, i32, i32, i32, i32, vp]
    lib.mmf_whisper_feature_window.argtypes = [vp, vp, i32, i32, i32, i32, vp]
    lib.mmf_whisper_gelu_window.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]
    lib.mmf_whisper_stem_out.argtypes = [vp, vp, vp, vp, i64, i32, i32, vp]
    S2 = C.c_int64 * 2
    lib.mmf_gemm_f32_grouped.argtypes = [C.POINTER(GemmProblem), i32, i32, i32, f32, vp]
    lib.mmf_gemm_f32_batched.argtypes = [C.POINTER(GemmProblem), i32, i32, f32, i32, i32, S2, S2, S2, vp]
    lib.mmf_softmax_rows_f32.argtypes = [vp, i64, i32, f32, vp]
    lib.mmf_softmax_bwd_rows_f32.argtypes = [vp, vp, i64, i32, f32, vp]
    lib.mmf_layernorm_f32_fwd.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, f32, vp]
    lib.mmf_layernorm_f32_bwd.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, vp]
    for name in SYMBOLS:
        getattr(lib, name)          # AttributeError here = header and .so disagree
    if lib.mmf_version() != 1:
        raise RuntimeError(f"libmmfusion ABI version {lib.mmf_version()} != 1")
    _lib = lib
    if os.environ.get("MMF_GEMM_IMPL"):    # A/B runs: pin a GEMM kernel generation for the whole process
        check(lib.mmf_gemm_select_impl(int(os.environ["MMF_GEMM_IMPL"])))
    return lib


def check(rc: int) -> None:
    if rc != 0:
        raise RuntimeError(f"libmmfusion error {rc}: {load().mmf_last_error().decode()}")


def stream_ptr() -> int:
    """The HIP stream torch is currently enqueuing on (raw hipStream_t)."""
    import torch
    return torch.cuda.current_stream().cuda_stream


# ---- optional launch timing (bench.py's roofline leg) --------------------------------------------
# When PROFILE is a list, every grouped GEMM / attention launch is bracketed by HIP events recorded
# on the launch stream and appended as (kernel label, algorithmic flops, start, end).
PROFILE: Optional[list] = None
_LAYOUT_NAME = {GEMM_NT: "NT", GEMM_NN: "NN", GEMM_TN: "TN"}


class _Timed:
    def __init__(self, label: str, flops: float, detail=None):
        self.label, self.flops, self.detail = label, flops, detail

    def __enter__(self):
        if PROFILE is not None:
            import torch
            self.e0, self.e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            self.e0.record(torch.cuda.current_stream())
        return self

    def __exit__(self, *exc):
        if PROFILE is not None:
            import torch
            self.e1.record(torch.cuda.current_stream())
            PROFILE.append((self.label, self.flops, self.e0, self.e1, self.detail))


def gemm_grouped(problems: Sequence[GemmProblem], layout: int, epilogue: int, out_f32: bool,
                 alpha: float = 1.0, dropout_p: float = 0.0, rng_state_ptr: Optional[int] = None, site: int = 0) -> None:
    arr = (GemmProblem * len(problems))(*problems)
    flops = sum(2.0 * p.M * p.N * p.K for p in problems) if PROFILE is not None else 0.0
    detail = [(p.M, p.N, p.K) for p in problems] if PROFILE is not None else None
    with _Timed(f"gemm_grouped_kernel<{_LAYOUT_NAME[layout]},{'f32' if out_f32 else 'bf16'}>", flops, detail) as tm:
        if alpha == 1.0 and not (epilogue & EPI_DROPOUT):
            check(load().mmf_gemm_grouped(arr, len(problems), layout, epilogue, int(out_f32), stream_ptr()))
        else:
            ex = GemmExtra(alpha, dropout_p, rng_state_ptr, site)
            check(load().mmf_gemm_grouped_ex(arr, len(problems), layout, epilogue, int(out_f32), C.byref(ex), stream_ptr()))
        if PROFILE is not None:            # name the kernel generation that ran: the dominant kernel is a kernel symbol
            tm.label = f"gemm{load().mmf_gemm_last_impl()}_grouped_kernel<{_LAYOUT_NAME[layout]},{'f32' if out_f32 else 'bf16'}>"


def gemm_relu_bits_available(problems: Sequence[GemmProblem], layout: int, epilogue: int, alpha: float = 1.0,
                             dropout_p: float = 0.0, rng_state_ptr: Optional[int] = None, site: int = 0) -> bool:
    """Whether ``gemm_grouped`` with these arguments (a bf16-output launch whose epilogue holds EPI_RELU_BITS or
    EPI_MASK_BITS) would run on the persistent kernel, the only one with the bit forms.  Host only."""
    arr = (GemmProblem * len(problems))(*problems)
    ex = GemmExtra(alpha, dropout_p, rng_state_ptr, site)
    return bool(load().mmf_gemm_relu_bits_available(arr, len(problems), layout, epilogue, 0, C.byref(ex)))


def gemm_chain_available(chains: Sequence[GemmChain], layout: int, epilogue: int) -> bool:
    """Whether ``gemm_grouped_chain`` takes exactly this launch (``mmf_gemm_chain_available``).  Host only."""
    if not 0 < len(chains) <= GEMM_MAX_CHAINS:
        return False
    arr = (GemmChain * len(chains))(*chains)
    return bool(load().mmf_gemm_chain_available(arr, len(chains), layout, epilogue, None))


def gemm_grouped_chain(chains: Sequence[GemmChain], layout: int, epilogue: int) -> None:
    """One launch of K-segment chains: every chain's output is the sum of its segments' products, accumulated in one
    MFMA chain per output tile and stored once (``mmf_gemm_grouped_chain``)."""
    arr = (GemmChain * len(chains))(*chains)
    flops = sum(2.0 * c.M * c.N * c.seg[j].K for c in chains for j in range(c.num_segments)) if PROFILE is not None else 0.0
    detail = [(c.M, c.N, sum(c.seg[j].K for j in range(c.num_segments))) for c in chains] if PROFILE is not None else None
    with _Timed(f"gemm7_chain_kernel<{_LAYOUT_NAME[layout]},bf16>", flops, detail):
        check(load().mmf_gemm_grouped_chain(arr, len(chains), layout, epilogue, stream_ptr()))


def _attn_call(label: str, factor: float, problems: Sequence[AttnProblem], head_dim: int, entry: str, *args) -> None:
    """One grouped-attention call ``entry(problems, n, head_dim, *args, stream)`` inside its ``_Timed`` bracket ``label<head_dim>``.
    ``factor``: the pass's algorithmic FLOPs per B*H*Tq*Tk*head_dim — 4 for the forward (S, P.V), 8 for the backward (dV, dP, dQ,
    dK), 4 for the uniform backward (dQ, dK) and for delta (S, dP); the recomputed S of a backward is not credited."""
    arr = (AttnProblem * len(problems))(*problems)
    flops = sum(factor * p.B * p.H * p.Tq * p.Tk * head_dim for p in problems) if PROFILE is not None else 0.0
    with _Timed(f"{label}<{head_dim}>", flops, [(p.Tq, p.Tk) for p in problems] if PROFILE is not None else None):
        check(getattr(load(), entry)(arr, len(problems), head_dim, *args, stream_ptr()))


def attn_fwd_grouped(problems: Sequence[AttnProblem], head_dim: int, scale: float, dropout_p: float = 0.0,
                     rng_state_ptr: Optional[int] = None, site: int = 0) -> None:
    _attn_call("attn_fwd_kernel", 4.0, problems, head_dim, "mmf_attn_fwd_grouped_ex", scale, dropout_p, rng_state_ptr, site)


def attn_bwd_grouped(problems: Sequence[AttnProblem], head_dim: int, scale: float, dropout_p: float = 0.0,
                     rng_state_ptr: Optional[int] = None, site: int = 0) -> None:
    _attn_call("attn_bwd_kernels", 8.0, problems, head_dim, "mmf_attn_bwd_grouped_ex", scale, dropout_p, rng_state_ptr, site)


def attn_bwd_uniform_available(head_dim: int, dropout_p: float) -> bool:
    """whether ``attn_bwd_grouped_uniform`` has kernels for this head_dim and dropout (``mmf_attn_bwd_grouped_uniform_available``)"""
    return bool(load().mmf_attn_bwd_grouped_uniform_available(head_dim, dropout_p))


def attn_bwd_uniform_workspace_bytes(problems: Sequence[AttnProblem]) -> int:
    arr = (AttnProblem * len(problems))(*problems)
    return int(load().mmf_attn_bwd_grouped_uniform_workspace_bytes(arr, len(problems)))


def attn_bwd_grouped_uniform(problems: Sequence[AttnProblem], head_dim: int, scale: float, workspace, pooled=None) -> None:
    """the backward of attentions consumed through their mean over the queries: ``dO`` of every problem is the (B, ldo) matrix of
    one gradient row per batch row (include/mmfusion.h).  ``workspace``: a contiguous f32 tensor of at least
    ``attn_bwd_uniform_workspace_bytes(problems)`` bytes (it need not be initialised).  ``pooled`` = (pointers, lddy): per problem
    the (B, lddy) gradient of the pooled output, from which the launch itself writes those rows (``mmf_attn_bwd_grouped_pooled``)."""
    ws = (workspace.data_ptr(), workspace.numel() * workspace.element_size())
    if pooled is None:
        _attn_call("attn_bwd_uniform_kernels", 4.0, problems, head_dim, "mmf_attn_bwd_grouped_uniform", scale, *ws)
    else:
        dys = (C.c_void_p * len(problems))(*pooled[0])
        _attn_call("attn_bwd_uniform_kernels", 4.0, problems, head_dim, "mmf_attn_bwd_grouped_pooled", scale, dys, pooled[1], *ws)


def attn_bwd_grouped_exact_delta(problems: Sequence[AttnProblem], head_dim: int, scale: float) -> None:
    """``attn_bwd_grouped`` (no dropout) with delta = sum_j p_ij dp_ij formed in f32 by ``mmf_attn_delta_f32`` instead of dO . O from
    the bf16 O: one more pass over the keys, for gradients that the rounding of O would otherwise bury (include/mmfusion.h)"""
    _attn_call("attn_delta_kernel", 4.0, problems, head_dim, "mmf_attn_delta_f32", scale)
    _attn_call("attn_bwd_kernels", 8.0, problems, head_dim, "mmf_attn_bwd_grouped_delta", scale)


def _drop_args(who: str, drop) -> tuple:
    """``drop`` = (p, state, site, base) -> the four trailing arguments of every entry point with keyed dropout: ``state`` the device
    int64 [1] RNG state (``ops.rng_state()``).  The one difference between callers is ``base``: for the per-item kernels it is the
    index in the whole batch of the call's first item (``item0``); for the grouped attention's ``_keyed`` entries it is the stream
    base, in (item, head) pairs (Wav2Vec2 passes ``item0 * H`` there)"""
    import torch
    p, state, site, base = drop
    if state is not None and (not state.is_cuda or state.dtype != torch.int64 or state.numel() != 1):
        raise ValueError(f"{who}: the dropout state must be one int64 on the GPU")
    return float(p), None if state is None else state.data_ptr(), int(site), int(base)


def attn_fwd_grouped_keyed(problems: Sequence[AttnProblem], head_dim: int, scale: float, drop) -> None:
    """``attn_fwd_grouped`` with dropout of the probabilities, ``drop`` = (p, state, site, stream_base): the stream id of (problem, b,
    h) is problem * 4096 + stream_base + b H + h (``mmf_attn_fwd_grouped_keyed``); lse stays the undropped one"""
    _attn_call("attn_fwd_kernel", 4.0, problems, head_dim, "mmf_attn_fwd_grouped_keyed", scale, *_drop_args("attn_fwd_grouped_keyed", drop))


def wavlm_gate(x, lin_w, lin_b, head_const, gate, n: int, T: int, H: int, head_dim: int) -> None:
    """WavLM's gate of the relative position bias (``mmf_wavlm_gate``): x (n T, H head_dim) bf16 rows, the layer's input ->
    gate (n, H, T) f32; lin_w (8, head_dim), lin_b (8), head_const (H) f32"""
    import torch
    if (x.dtype != torch.bfloat16 or x.dim() != 2 or x.stride(1) != 1 or x.shape[0] != n * T or x.shape[1] != H * head_dim
            or lin_w.numel() != 8 * head_dim or lin_b.numel() != 8 or head_const.numel() != H or gate.numel() < n * H * T
            or any(t.dtype != torch.float32 or not t.is_contiguous() for t in (lin_w, lin_b, head_const, gate))):
        raise ValueError("wavlm_gate: operand sizes do not match n, T, H, head_dim")
    with _Timed("wavlm_gate_kernel", 16.0 * n * T * H * head_dim, [(n * T, H * head_dim)]):
        check(load().mmf_wavlm_gate(x.data_ptr(), x.stride(0), lin_w.data_ptr(), lin_b.data_ptr(), head_const.data_ptr(),
                                    gate.data_ptr(), n, T, H, head_dim, stream_ptr()))


def attn_fwd_relbias(problem: AttnProblem, head_dim: int, scale: float, gate, table) -> None:
    """the fused self-attention forward with WavLM's gated relative position bias (``mmf_attn_fwd_relbias``): score = scale q . k +
    gate[b][h][i] table[h][j - i + T - 1]; gate (B, H, T) f32, table (H, 2T - 1) f32, both contiguous on the GPU"""
    import torch
    T = problem.Tq
    if (gate.dtype != torch.float32 or table.dtype != torch.float32 or not gate.is_contiguous() or not table.is_contiguous()
            or gate.numel() < problem.B * problem.H * T or table.numel() != problem.H * (2 * T - 1)):
        raise ValueError("attn_fwd_relbias: gate must hold (B, H, T) and table (H, 2T - 1) contiguous f32")
    flops = 4.0 * problem.B * problem.H * T * T * head_dim if PROFILE is not None else 0.0
    with _Timed(f"attn_fwd_relbias_kernel<{head_dim}>", flops, [(T, T)] if PROFILE is not None else None):
        check(load().mmf_attn_fwd_relbias(C.byref(problem), head_dim, scale, gate.data_ptr(), table.data_ptr(), stream_ptr()))


# ---- the BERT family's kernels (csrc/bert.hip) ---------------------------------------------------------------------
BERT_POSITIONS = {"bert": 0, "roberta": 1}            # mmf_bert_embed's position_rule


def mask_pack_words(T: int) -> int:
    """uint32 words of one item's row of ``mask_pack``'s output (``mmf_mask_pack_words``): one past the last valid key, the count
    of valid keys, then one bit per key in whole 64-key tiles"""
    return 2 + 2 * ((T + 63) // 64)


def mask_pack(mask, packed, n: int, T: int) -> None:
    """``mask`` (n, T) contiguous float32 / uint8 / bool on the GPU, or None for all ones -> ``packed``: int32, at least
    n * ``mask_pack_words(T)`` elements, as ``attn_fwd_keymask`` reads it (``mmf_mask_pack``; one launch, no host step)"""
    import torch
    if not packed.is_cuda or (mask is not None and not mask.is_cuda):
        raise RuntimeError("mask_pack runs on the GPU only (no CPU fallback)")
    if packed.dtype != torch.int32 or not packed.is_contiguous() or packed.numel() < n * mask_pack_words(T) or n < 1 or T < 1:
        raise ValueError("mask_pack: packed must be contiguous int32 with n * mask_pack_words(T) elements")
    mp, kind = None, 0
    if mask is not None:
        if mask.dtype not in (torch.float32, torch.uint8, torch.bool) or not mask.is_contiguous() or mask.numel() != n * T:
            raise ValueError("mask_pack: the mask must be a contiguous float32 / uint8 / bool tensor of n * T elements")
        mp, kind = mask.data_ptr(), 1 if mask.dtype == torch.float32 else 2
    with _Timed("mask_pack_kernel", 0.0, [(n, T)]):
        check(load().mmf_mask_pack(mp, kind, packed.data_ptr(), n, T, stream_ptr()))


def attn_fwd_keymask(problem: AttnProblem, head_dim: int, scale: float, packed) -> None:
    """the fused self-attention forward with a key padding mask (``mmf_attn_fwd_keymask``): ``packed`` holds the B items' rows as
    ``mask_pack`` writes them"""
    import torch
    T = problem.Tq
    if not packed.is_cuda:
        raise RuntimeError("attn_fwd_keymask runs on the GPU only (no CPU fallback)")
    if packed.dtype != torch.int32 or not packed.is_contiguous() or packed.numel() < problem.B * mask_pack_words(T):
        raise ValueError("attn_fwd_keymask: packed must be contiguous int32 with B * mask_pack_words(T) elements")
    flops = 4.0 * problem.B * problem.H * T * T * head_dim if PROFILE is not None else 0.0
    with _Timed(f"attn_fwd_keymask_kernel<{head_dim}>", flops, [(T, T)] if PROFILE is not None else None):
        check(load().mmf_attn_fwd_keymask(C.byref(problem), head_dim, scale, packed.data_ptr(), stream_ptr()))


def bert_embed(out, word, pos, type_table, gamma, beta, eps: float, T: int, rule: str, pad: int = 0, ids=None, embeds=None,
               token_type_ids=None) -> None:
    """out (rows, d) bf16 = LayerNorm((word[ids] | embeds) + type_table[token_type_ids] + pos[p]), rows = n * T (``mmf_bert_embed``).
    ``rule``: "bert" (p = the token's place) or "roberta" (from the ids and ``pad``; on the embeds route pad + 1 + place); ids /
    token_type_ids int64 (rows,), the latter optional (row 0); the tables f32 (vocab | positions | types, d)"""
    import torch
    _w2v_bf16(out)
    _w2v_f32(pos, type_table, gamma, beta)
    if (ids is None) == (embeds is None):
        raise ValueError("bert_embed: exactly one of ids / embeds")
    if rule not in BERT_POSITIONS:
        raise ValueError(f"bert_embed: rule {rule!r} is not one of {sorted(BERT_POSITIONS)}")
    if out.dim() != 2 or not out.is_contiguous():
        raise ValueError("bert_embed: out must be a contiguous (rows, d) matrix")
    rows, d = out.shape
    if T < 1 or rows % T or any(t.dim() != 2 or t.shape[1] != d for t in (pos, type_table)) or gamma.numel() != d or beta.numel() != d:
        raise ValueError("bert_embed: rows must be a multiple of T, the tables (.., d) and gamma / beta one value per column")
    for name, t in (("ids", ids), ("token_type_ids", token_type_ids)):
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("bert_embed runs on the GPU only (no CPU fallback)")
        if t.dtype != torch.int64 or not t.is_contiguous() or t.numel() != rows:
            raise ValueError(f"bert_embed: {name} must be contiguous int64, one per output row")
    vocab = 0
    if ids is not None:
        _w2v_f32(word)
        if word.dim() != 2 or word.shape[1] != d:
            raise ValueError("bert_embed: word must be (vocab, d)")
        vocab = word.shape[0]
    else:
        _w2v_f32(embeds)
        if embeds.numel() != rows * d:
            raise ValueError("bert_embed: embeds must hold (rows, d) values")
    ptr = lambda t: None if t is None else t.data_ptr()
    with _Timed("bert_embed_kernel", 0.0, [(rows, d)]):
        check(load().mmf_bert_embed(ptr(ids), ptr(embeds), ptr(token_type_ids), ptr(word) if ids is not None else None, pos.data_ptr(),
                                    type_table.data_ptr(), gamma.data_ptr(), beta.data_ptr(), eps, BERT_POSITIONS[rule], int(pad),
                                    out.data_ptr(), rows, T, d, vocab, pos.shape[0], type_table.shape[0], stream_ptr()))


def attn_delta_keyed(problems: Sequence[AttnProblem], head_dim: int, scale: float, drop) -> None:
    """delta = sum_j p_ij w_ij dp_ij in f32 under the mask of ``drop`` (``mmf_attn_delta_f32_keyed``)"""
    _attn_call("attn_delta_kernel", 4.0, problems, head_dim, "mmf_attn_delta_f32_keyed", scale, *_drop_args("attn_delta_keyed", drop))


def attn_bwd_grouped_delta_keyed(problems: Sequence[AttnProblem], head_dim: int, scale: float, drop) -> None:
    """the backward from a given delta under the mask of ``drop`` (``mmf_attn_bwd_grouped_delta_keyed``)"""
    _attn_call("attn_bwd_kernels", 8.0, problems, head_dim, "mmf_attn_bwd_grouped_delta_keyed", scale,
               *_drop_args("attn_bwd_grouped_delta_keyed", drop))


def attn_bwd_grouped_exact_delta_keyed(problems: Sequence[AttnProblem], head_dim: int, scale: float, drop) -> None:
    """``attn_bwd_grouped_exact_delta`` with the forward's dropout mask drawn again in all three kernels"""
    attn_delta_keyed(problems, head_dim, scale, drop)
    attn_bwd_grouped_delta_keyed(problems, head_dim, scale, drop)


def layernorm_fwd_grouped(problems: Sequence[LnProblem], d: int, eps: float) -> None:
    arr = (LnProblem * len(problems))(*problems)
    check(load().mmf_layernorm_fwd_grouped(arr, len(problems), d, eps, stream_ptr()))


def layernorm2_add3_available(rows: Sequence[int], d: int) -> bool:
    """Whether the fused norm2 + three-way sum applies to sums of these row counts: d is a lane width and the separate
    LayerNorm forward over the same rows would take the lane form too (the launch is then bit-equal to the two it replaces)."""
    arr = (C.c_int32 * len(rows))(*rows)
    return bool(load().mmf_layernorm2_add3_available(arr, len(rows), d))


def layernorm2_add3_fwd_grouped(problems: Sequence[Ln2Add3Problem], d: int, eps: float) -> None:
    arr = (Ln2Add3Problem * len(problems))(*problems)
    check(load().mmf_layernorm2_add3_fwd_grouped(arr, len(problems), d, eps, stream_ptr()))


def layernorm_bwd_grouped(problems: Sequence[LnProblem], d: int, workspace) -> None:
    """workspace: a float32 torch tensor of >= mmf_layernorm_bwd_workspace_bytes(d) bytes."""
    arr = (LnProblem * len(problems))(*problems)
    check(load().mmf_layernorm_bwd_grouped(arr, len(problems), d, workspace.data_ptr(),
                                           workspace.numel() * workspace.element_size(), stream_ptr()))


def layernorm_bwd_add_grouped(problems: Sequence[LnProblem], d: int, workspace) -> None:
    """``layernorm_bwd_grouped`` with dx = r + the input gradient, r the bf16 rows behind each problem's ``y`` (it may be dx)."""
    arr = (LnProblem * len(problems))(*problems)
    check(load().mmf_layernorm_bwd_add_grouped(arr, len(problems), d, workspace.data_ptr(),
                                               workspace.numel() * workspace.element_size(), stream_ptr()))


SUM_SLABS_MAX = 64               # MMF_SUM_SLABS_MAX of include/mmfusion.h


def sum_slabs(partial, out, accumulate: bool) -> None:
    """out (f32, contiguous) = (out if ``accumulate`` else 0) + partial[0] + ... + partial[S - 1] in that order; partial (S, numel of
    out) f32 contiguous"""
    import torch
    if partial.dtype != torch.float32 or out.dtype != torch.float32 or not partial.is_contiguous() or not out.is_contiguous() \
            or partial.dim() != 2 or partial.shape[1] != out.numel():
        raise ValueError("sum_slabs: partial must be contiguous f32 (slabs, out.numel()) and out contiguous f32")
    with _Timed("sum_slabs_kernel", 0.0, [(partial.shape[0], out.numel())]):
        check(load().mmf_sum_slabs_f32(partial.data_ptr(), out.data_ptr(), out.numel(), partial.shape[0], int(bool(accumulate)), stream_ptr()))


def colsum_grouped(problems: Sequence[ColsumProblem]) -> None:
    for i in range(0, len(problems), COLSUM_MAX_PROBLEMS):
        chunk = problems[i:i + COLSUM_MAX_PROBLEMS]
        arr = (ColsumProblem * len(chunk))(*chunk)
        check(load().mmf_colsum_grouped(arr, len(chunk), stream_ptr()))


def skinny_fwd(problems: Sequence[SkinnyProblem], flags: int, out_f32: bool) -> None:
    for i in range(0, len(problems), SKINNY_MAX_PROBLEMS):
        chunk = problems[i:i + SKINNY_MAX_PROBLEMS]
        arr = (SkinnyProblem * len(chunk))(*chunk)
        check(load().mmf_skinny_linear_fwd(arr, len(chunk), flags, int(out_f32), stream_ptr()))


def skinny_fwd_ex(problems: Sequence[SkinnyProblemEx], flags: int, out_f32: bool, extra: SkinnyExtra) -> None:
    """one launch: the group must fit (a dropout group's problem index keys its masks)"""
    if len(problems) > SKINNY_MAX_PROBLEMS:
        raise ValueError("a fused row-linear group must fit one launch")
    arr = (SkinnyProblemEx * len(problems))(*problems)
    check(load().mmf_skinny_linear_fwd_ex(arr, len(problems), flags, int(out_f32), C.byref(extra), stream_ptr()))


def skinny_dgrad_ex(problems: Sequence[SkinnyProblemEx], flags: int, alpha: float, out_f32: bool, extra: SkinnyExtra) -> None:
    if len(problems) > SKINNY_MAX_PROBLEMS:
        raise ValueError("a fused row-linear group must fit one launch")
    arr = (SkinnyProblemEx * len(problems))(*problems)
    check(load().mmf_skinny_linear_dgrad_ex(arr, len(problems), flags, alpha, int(out_f32), C.byref(extra), stream_ptr()))


def skinny_dgrad(problems: Sequence[SkinnyProblem], flags: int, alpha: float, out_f32: bool) -> None:
    for i in range(0, len(problems), SKINNY_MAX_PROBLEMS):
        chunk = problems[i:i + SKINNY_MAX_PROBLEMS]
        arr = (SkinnyProblem * len(chunk))(*chunk)
        check(load().mmf_skinny_linear_dgrad(arr, len(chunk), flags, alpha, int(out_f32), stream_ptr()))


# ---- ViT streaming kernels (csrc/vit.hip); tensors, not pointers: the shapes are checked here ---------------
def vit_patchify(pixels, patches, N: int, C: int, H: int, W: int, P: int) -> None:
    """pixels (N, C, H, W) f32 contiguous -> patches (N * (H/P) * (W/P), C*P*P) bf16 contiguous"""
    if pixels.numel() != N * C * H * W or not pixels.is_contiguous() or not patches.is_contiguous() \
            or patches.numel() != pixels.numel():
        raise ValueError("vit_patchify: pixels / patches do not hold N x C x H x W contiguous elements")
    with _Timed("vit_patchify_kernel", 0.0, [(N, C * H * W)]):
        check(load().mmf_vit_patchify(pixels.data_ptr(), patches.data_ptr(), N, C, H, W, P, stream_ptr()))


def vit_embed_tokens(patch_emb, cls, pos, tokens, N: int, T: int, d: int) -> None:
    if patch_emb.numel() != N * (T - 1) * d or not patch_emb.is_contiguous() or cls.numel() != d or pos.numel() != T * d \
            or tokens.numel() < N * T * d or not tokens.is_contiguous():
        raise ValueError("vit_embed_tokens: operand sizes do not match N, T, d")
    with _Timed("vit_embed_tokens_kernel", 0.0, [(N * T, d)]):
        check(load().mmf_vit_embed_tokens(patch_emb.data_ptr(), cls.data_ptr(), pos.data_ptr(), tokens.data_ptr(), N, T, d,
                                          stream_ptr()))


def vit_embed_tokens_bwd(dtokens, dcls, dpos, dpatch_emb, N: int, T: int, d: int) -> None:
    """dtokens (N T, d) bf16 -> dcls (d) f32 += its rows n T summed over n, dpos (T, d) f32 += its rows summed over n per position,
    dpatch_emb (N (T - 1), d) bf16 = its rows 1 .. T - 1 of every image"""
    if dtokens.numel() != N * T * d or not dtokens.is_contiguous() or dcls.numel() != d or dpos.numel() != T * d \
            or dpatch_emb.numel() != N * (T - 1) * d or not dpatch_emb.is_contiguous() or not dcls.is_contiguous() or not dpos.is_contiguous():
        raise ValueError("vit_embed_tokens_bwd: operand sizes do not match N, T, d")
    with _Timed("vit_embed_tokens_bwd_kernel", 0.0, [(N * T, d)]):
        check(load().mmf_vit_embed_tokens_bwd(dtokens.data_ptr(), dcls.data_ptr(), dpos.data_ptr(), dpatch_emb.data_ptr(), N, T, d,
                                              stream_ptr()))


def vit_cls_attn_bwd(qkv, dout, dqkv, N: int, H: int, T: int, head_dim: int, scale: float) -> None:
    """qkv (N T, 3 H head_dim) bf16 fused rows, dout (N, H head_dim) bf16 -> dqkv laid out as qkv: the backward of the attention
    of row 0 of each image over its T keys (dq on row 0, dk | dv on every row)"""
    d = H * head_dim
    if tuple(qkv.shape) != (N * T, 3 * d) or tuple(dqkv.shape) != (N * T, 3 * d) or tuple(dout.shape) != (N, d) \
            or not (qkv.is_contiguous() and dqkv.is_contiguous() and dout.is_contiguous()):
        raise ValueError("vit_cls_attn_bwd: operand shapes do not match N, H, T, head_dim")
    with _Timed("vit_cls_attn_bwd_kernel", 0.0, [(N * T, 2 * d)]):
        check(load().mmf_vit_cls_attn_bwd(qkv.data_ptr(), dout.data_ptr(), dqkv.data_ptr(), N, H, T, head_dim, scale, stream_ptr()))


def bias_gelu(x, bias=None) -> None:
    """x (rows, cols) bf16, row-strided allowed, in place: gelu(x + bias), the exact form v Phi(v) with Phi through erfc"""
    if x.dim() != 2 or x.stride(1) != 1 or (bias is not None and (bias.numel() != x.shape[1] or not bias.is_contiguous())):
        raise ValueError("bias_gelu: x must be 2-D with contiguous rows and bias one value per column")
    with _Timed("bias_gelu_kernel", 0.0, [tuple(x.shape)]):
        check(load().mmf_bias_gelu_bf16(x.data_ptr(), bias.data_ptr() if bias is not None else None, x.shape[0], x.shape[1],
                                        x.stride(0), stream_ptr()))


def _gelu_blocks(who: str, bias, *ts) -> None:
    """2-D bf16 blocks of one shape and one row stride, contiguous rows; bias one f32 value per column or None"""
    x = ts[0]
    if any(t.dim() != 2 or t.stride(1) != 1 or t.shape != x.shape or t.stride(0) != x.stride(0) for t in ts) or (
            bias is not None and (bias.numel() != x.shape[1] or not bias.is_contiguous())):
        raise ValueError(f"{who}: 2-D blocks of one shape and row stride with contiguous rows, and bias one value per column")


def bias_gelu_to(h, bias, g) -> None:
    """g <- gelu(h + bias), h kept: the out-of-place form of ``bias_gelu``, bit-identical to it"""
    _gelu_blocks("bias_gelu_to", bias, h, g)
    with _Timed("bias_gelu_kernel", 0.0, [tuple(h.shape)]):
        check(load().mmf_bias_gelu_bf16_to(h.data_ptr(), bias.data_ptr() if bias is not None else None, g.data_ptr(), h.shape[0],
                                           h.shape[1], h.stride(0), stream_ptr()))


def bias_gelu_bwd(dg, h, bias, dh) -> None:
    """dh <- dg * gelu'(h + bias); ``h`` the stored linear output before its bias; ``dh`` may be ``dg``"""
    _gelu_blocks("bias_gelu_bwd", bias, dg, h, dh)
    with _Timed("bias_gelu_bwd_kernel", 0.0, [tuple(h.shape)]):
        check(load().mmf_bias_gelu_bwd_bf16(dg.data_ptr(), h.data_ptr(), bias.data_ptr() if bias is not None else None, dh.data_ptr(),
                                            h.shape[0], h.shape[1], h.stride(0), stream_ptr()))


# ---- Wav2Vec2 kernels (csrc/wav2vec2.hip); tensors, not pointers: the shapes are checked here --------------
W2V_STATS_SLOTS = 128            # MMF_W2V_STATS_SLOTS of include/mmfusion.h (tests/test_w2v_cpu.py compares the two)


def _w2v_f32(*ts) -> None:
    import torch
    for t in ts:
        if not t.is_cuda:
            raise RuntimeError("w2v kernels run on the GPU only (no CPU fallback)")
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("w2v: the f32 operands must be contiguous float32 tensors")


def _w2v_bf16(*ts) -> None:
    import torch
    for t in ts:
        if not t.is_cuda:
            raise RuntimeError("w2v kernels run on the GPU only (no CPU fallback)")
        if t.dtype != torch.bfloat16:
            raise TypeError(f"w2v: expected a bfloat16 operand, got {t.dtype}")


def w2v_conv0_stats(wave, weight, stats, partial, k0: int, s0: int) -> None:
    """wave (N, L) f32, weight (C0, 1, k0) f32 -> stats (N, 2, C0) f32: mean and biased variance of the layer-0 convolution
    per (clip, channel); partial: N * W2V_STATS_SLOTS * 2 * C0 floats of scratch"""
    _w2v_f32(wave, weight, stats, partial)
    N, L = wave.shape
    C0 = weight.shape[0]
    if weight.numel() != C0 * k0 or stats.numel() < N * 2 * C0 or partial.numel() < N * W2V_STATS_SLOTS * 2 * C0:
        raise ValueError("w2v_conv0_stats: operand sizes do not match N, C0, k0")
    with _Timed("w2v_conv0_stats_kernels", 2.0 * N * ((L - k0) // s0 + 1) * C0 * k0, [(N, L)]):
        check(load().mmf_w2v_conv0_stats(wave.data_ptr(), weight.data_ptr(), stats.data_ptr(), partial.data_ptr(), N, L, C0, k0, s0,
                                         stream_ptr()))


def w2v_conv0_norm_gelu(wave, weight, stats, gamma, beta, out, k0: int, s0: int, k1: int, s1: int, eps: float) -> None:
    """-> out (N, T1, k1 * C0) bf16: gelu(groupnorm(conv0(wave))) in the window form of the next conv layer"""
    _w2v_f32(wave, weight, stats, gamma, beta)
    _w2v_bf16(out)
    N, L = wave.shape
    C0 = weight.shape[0]
    T1 = (((L - k0) // s0 + 1) - k1) // s1 + 1
    if weight.numel() != C0 * k0 or stats.numel() < N * 2 * C0 or gamma.numel() != C0 or beta.numel() != C0 \
            or T1 < 1 or out.numel() < N * T1 * k1 * C0 or not out.is_contiguous():
        raise ValueError("w2v_conv0_norm_gelu: operand sizes do not match N, L, C0 and the two kernels")
    with _Timed("w2v_conv0_norm_gelu_kernel", 2.0 * N * ((L - k0) // s0 + 1) * C0 * k0, [(N, L)]):
        check(load().mmf_w2v_conv0_norm_gelu(wave.data_ptr(), weight.data_ptr(), stats.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                             out.data_ptr(), N, L, C0, k0, s0, k1, s1, eps, stream_ptr()))


def w2v_gelu_window(x, out, N: int, T_in: int, C: int, k: int, s: int) -> None:
    """x (N, T_in, C) bf16 -> out (N, T_out, k * C) bf16, out[n][t][j*C + c] = gelu(x[n][s*t + j][c])"""
    _w2v_bf16(x, out)
    T_out = (T_in - k) // s + 1
    if x.numel() < N * T_in * C or not x.is_contiguous() or T_out < 1 or out.numel() < N * T_out * k * C or not out.is_contiguous():
        raise ValueError("w2v_gelu_window: operand sizes do not match N, T_in, C, k, s")
    with _Timed("w2v_gelu_window_kernel", 0.0, [(N * T_out, k * C)]):
        check(load().mmf_w2v_gelu_window(x.data_ptr(), out.data_ptr(), N, T_in, C, k, s, stream_ptr()))


def w2v_conv0_ln_gelu(wave, weight, bias, gamma, beta, out, k0: int, s0: int, k1: int, s1: int, eps: float) -> None:
    """-> out (N, T1, k1 * C0) bf16: gelu(layernorm over channels(conv0(wave) + bias)) in the window form of the next conv layer, one
    pass (``mmf_w2v_conv0_ln_gelu``); ``bias`` None: none"""
    _w2v_f32(wave, weight, gamma, beta, *(() if bias is None else (bias,)))
    _w2v_bf16(out)
    N, L = wave.shape
    C0 = weight.shape[0]
    T1 = (((L - k0) // s0 + 1) - k1) // s1 + 1
    if weight.numel() != C0 * k0 or gamma.numel() != C0 or beta.numel() != C0 or (bias is not None and bias.numel() != C0) \
            or T1 < 1 or out.numel() < N * T1 * k1 * C0 or not out.is_contiguous():
        raise ValueError("w2v_conv0_ln_gelu: operand sizes do not match N, L, C0 and the two kernels")
    with _Timed("w2v_conv0_ln_gelu_kernel", 2.0 * N * ((L - k0) // s0 + 1) * C0 * k0, [(N, L)]):
        check(load().mmf_w2v_conv0_ln_gelu(wave.data_ptr(), weight.data_ptr(), None if bias is None else bias.data_ptr(), gamma.data_ptr(),
                                           beta.data_ptr(), out.data_ptr(), N, L, C0, k0, s0, k1, s1, eps, stream_ptr()))


def w2v_ln_gelu_window(x, gamma, beta, out, N: int, T_in: int, C: int, k: int, s: int, eps: float) -> None:
    """x (N, T_in, C) bf16 -> out (N, T_out, k * C) bf16, out[n][t][j*C + c] = gelu(LN(x[n][s*t + j])[c]), LayerNorm over the channels
    of a row (``mmf_w2v_ln_gelu_window``); ``k == 0``: out (N, T_in, C), which may be x"""
    _w2v_bf16(x, out)
    _w2v_f32(gamma, beta)
    rows = ((T_in - k) // s + 1) * k if k else T_in
    if x.numel() < N * T_in * C or not x.is_contiguous() or rows < 1 or out.numel() < N * rows * C or not out.is_contiguous() \
            or gamma.numel() != C or beta.numel() != C:
        raise ValueError("w2v_ln_gelu_window: operand sizes do not match N, T_in, C, k, s")
    with _Timed("w2v_ln_gelu_window_kernel", 0.0, [(N * rows, C)]):
        check(load().mmf_w2v_ln_gelu_window(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(), N, T_in, C, k, s, eps, stream_ptr()))


def w2v_window_fold_gelu_bwd(dwin, x, dx, N: int, T_in: int, C: int, k: int, s: int) -> None:
    """dwin (N, T_out, k * C) bf16, the gradient of ``w2v_gelu_window``'s output, and its raw input x (N, T_in, C) bf16 -> dx like x:
    gelu'(x) times the fold of dwin, zeros on the frames no window reads; dx may be x"""
    _w2v_bf16(dwin, x, dx)
    T_out = (T_in - k) // s + 1
    if T_out < 1 or dwin.numel() < N * T_out * k * C or x.numel() < N * T_in * C or dx.numel() < N * T_in * C \
            or not (dwin.is_contiguous() and x.is_contiguous() and dx.is_contiguous()):
        raise ValueError("w2v_window_fold_gelu_bwd: operand sizes do not match N, T_in, C, k, s")
    with _Timed("w2v_window_fold_gelu_bwd_kernel", 0.0, [(N * T_in, C)]):
        check(load().mmf_w2v_window_fold_gelu_bwd(dwin.data_ptr(), x.data_ptr(), dx.data_ptr(), N, T_in, C, k, s, stream_ptr()))


def _w2v_conv0_bwd_sizes(who: str, wave, weight, stats, gamma, beta, dwin1, sums, k0: int, s0: int, k1: int, s1: int) -> tuple:
    _w2v_f32(wave, weight, stats, gamma, beta, sums)
    _w2v_bf16(dwin1)
    N, L = wave.shape
    C0 = weight.shape[0]
    T0 = (L - k0) // s0 + 1
    T1 = (T0 - k1) // s1 + 1
    if weight.numel() != C0 * k0 or stats.numel() < N * 2 * C0 or sums.numel() < N * 2 * C0 or gamma.numel() != C0 or beta.numel() != C0 \
            or T1 < 1 or dwin1.numel() < N * T1 * k1 * C0 or not dwin1.is_contiguous():
        raise ValueError(f"{who}: operand sizes do not match N, L, C0 and the two kernels")
    return N, L, C0, T0


def w2v_conv0_bwd_stats(wave, weight, stats, gamma, beta, dwin1, sums, partial, dgamma, dbeta, k0: int, s0: int, k1: int, s1: int,
                        eps: float, accumulate: bool = True) -> None:
    """layer 0's backward, pass 1 (``mmf_w2v_conv0_bwd_stats``): dwin1 (N, T1, k1 * C0) bf16, the gradient of
    ``w2v_conv0_norm_gelu``'s output -> sums (N, 2, C0) f32 = sum_t dy | sum_t dy xhat, and dgamma / dbeta (C0) f32 (+)= their sums
    over the clips; partial: N * W2V_STATS_SLOTS * 2 * C0 floats of scratch"""
    N, L, C0, _ = _w2v_conv0_bwd_sizes("w2v_conv0_bwd_stats", wave, weight, stats, gamma, beta, dwin1, sums, k0, s0, k1, s1)
    _w2v_f32(partial, dgamma, dbeta)
    if partial.numel() < N * W2V_STATS_SLOTS * 2 * C0 or dgamma.numel() != C0 or dbeta.numel() != C0:
        raise ValueError("w2v_conv0_bwd_stats: partial / dgamma / dbeta do not match N, C0")
    with _Timed("w2v_conv0_bwd_stats_kernels", 2.0 * N * ((L - k0) // s0 + 1) * C0 * k0, [(N, L)]):
        check(load().mmf_w2v_conv0_bwd_stats(wave.data_ptr(), weight.data_ptr(), stats.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                             dwin1.data_ptr(), sums.data_ptr(), partial.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(),
                                             N, L, C0, k0, s0, k1, s1, eps, int(bool(accumulate)), stream_ptr()))


def w2v_conv0_bwd_wgrad(wave, weight, stats, gamma, beta, dwin1, sums, partial, dweight, k0: int, s0: int, k1: int, s1: int, eps: float,
                        accumulate: bool = True) -> None:
    """layer 0's backward, pass 2 (``mmf_w2v_conv0_bwd_wgrad``): dweight (C0, 1, k0) f32 (+)= the convolution's weight gradient over
    all T0 frames of the N clips, from pass 1's ``sums``; partial: N * W2V_STATS_SLOTS * C0 * k0 floats of scratch"""
    N, L, C0, T0 = _w2v_conv0_bwd_sizes("w2v_conv0_bwd_wgrad", wave, weight, stats, gamma, beta, dwin1, sums, k0, s0, k1, s1)
    _w2v_f32(partial, dweight)
    if partial.numel() < N * W2V_STATS_SLOTS * C0 * k0 or dweight.numel() != C0 * k0:
        raise ValueError("w2v_conv0_bwd_wgrad: partial / dweight do not match N, C0, k0")
    with _Timed("w2v_conv0_bwd_wgrad_kernels", 4.0 * N * T0 * C0 * k0, [(N, L)]):
        check(load().mmf_w2v_conv0_bwd_wgrad(wave.data_ptr(), weight.data_ptr(), stats.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                             dwin1.data_ptr(), sums.data_ptr(), partial.data_ptr(), dweight.data_ptr(), N, L, C0, k0, s0,
                                             k1, s1, eps, int(bool(accumulate)), stream_ptr()))


def w2v_posconv(x, w, bias, y, N: int, T: int, C: int, groups: int, k: int) -> None:
    """y = x + gelu(grouped_conv(x) + bias) on (N, T, C) bf16; w (groups, C / groups, Kp) bf16 repacked (include/mmfusion.h)"""
    _w2v_bf16(x, w, y)
    _w2v_f32(bias)
    cg = C // max(groups, 1)
    Kp = (k * cg + 31) // 32 * 32
    if x.numel() < N * T * C or y.numel() < N * T * C or w.numel() != C * Kp or bias.numel() != C or not (
            x.is_contiguous() and y.is_contiguous() and w.is_contiguous() and bias.is_contiguous()):
        raise ValueError("w2v_posconv: operand sizes do not match N, T, C, groups, k")
    with _Timed("w2v_posconv_kernel", 2.0 * N * T * C * cg * k, [(N * T, C, k * cg)]):
        check(load().mmf_w2v_posconv(x.data_ptr(), w.data_ptr(), bias.data_ptr(), y.data_ptr(), N, T, C, groups, k, stream_ptr()))


def _w2v_posconv_sizes(what: str, acts, w, N: int, T: int, C: int, groups: int, k: int) -> int:
    """the shared size check of the positional convolution's backward wrappers -> cg"""
    cg = C // max(groups, 1)
    Kp = (k * cg + 31) // 32 * 32
    if any(t.numel() < N * T * C or not t.is_contiguous() for t in acts) or (w is not None and (w.numel() != C * Kp or not w.is_contiguous())):
        raise ValueError(f"{what}: operand sizes do not match N, T, C, groups, k")
    return cg


def w2v_posconv_bwd_act(x, w, bias, dy, dz, N: int, T: int, C: int, groups: int, k: int) -> None:
    """dz = dy * gelu'(grouped_conv(x) + bias) on (N, T, C) bf16: the pre-activation is computed again, as ``w2v_posconv`` does"""
    _w2v_bf16(x, w, dy, dz)
    _w2v_f32(bias)
    cg = _w2v_posconv_sizes("w2v_posconv_bwd_act", (x, dy, dz), w, N, T, C, groups, k)
    if bias.numel() != C:
        raise ValueError("w2v_posconv_bwd_act: operand sizes do not match N, T, C, groups, k")
    with _Timed("w2v_posconv_bwd_act_kernel", 2.0 * N * T * C * cg * k, [(N * T, C, k * cg)]):
        check(load().mmf_w2v_posconv_bwd_act(x.data_ptr(), w.data_ptr(), bias.data_ptr(), dy.data_ptr(), dz.data_ptr(), N, T, C, groups, k,
                                             stream_ptr()))


def w2v_posconv_dgrad(dz, wt, dy, dx, N: int, T: int, C: int, groups: int, k: int) -> None:
    """dx = dy + the convolution's input gradient of dz on (N, T, C) bf16; wt: the packed weight with the taps reversed and
    co / ci swapped (include/mmfusion.h)"""
    _w2v_bf16(dz, wt, dy, dx)
    cg = _w2v_posconv_sizes("w2v_posconv_dgrad", (dz, dy, dx), wt, N, T, C, groups, k)
    with _Timed("w2v_posconv_dgrad_kernel", 2.0 * N * T * C * cg * k, [(N * T, C, k * cg)]):
        check(load().mmf_w2v_posconv_dgrad(dz.data_ptr(), wt.data_ptr(), dy.data_ptr(), dx.data_ptr(), N, T, C, groups, k, stream_ptr()))


def w2v_posconv_wgrad(dz, x, dw, N: int, T: int, C: int, groups: int, k: int, slabs: int = 1, accumulate: bool = False) -> None:
    """dw (C, Kp) f32, the packed layout of ``w2v_posconv``'s weight, (+)= the weight gradient over the N clips; ``slabs`` > 1:
    dw is (slabs, C, Kp), one partial per run of (clip, 128-row block) units, written, for ``sum_slabs``"""
    _w2v_bf16(dz, x)
    _w2v_f32(dw)
    cg = _w2v_posconv_sizes("w2v_posconv_wgrad", (dz, x), None, N, T, C, groups, k)
    if dw.numel() != max(slabs, 1) * C * ((k * cg + 31) // 32 * 32):
        raise ValueError("w2v_posconv_wgrad: dw is not (slabs, C, Kp)")
    with _Timed("w2v_posconv_wgrad_kernel", 2.0 * N * T * C * cg * k, [(N * T, C, k * cg)]):
        check(load().mmf_w2v_posconv_wgrad(dz.data_ptr(), x.data_ptr(), dw.data_ptr(), N, T, C, groups, k, slabs, int(bool(accumulate)),
                                           stream_ptr()))


def w2v_weightnorm_bwd(dw, g, v, dg, dv, overwrite_v: bool) -> None:
    """dw (C, Kp) f32, the packed gradient of the effective weight g v / ||v|| -> dg (1, 1, k) += , dv (C, cg, k) = or +="""
    _w2v_f32(dw, g, v, dg, dv)
    C, cg, k = v.shape
    if dw.numel() != C * ((k * cg + 31) // 32 * 32) or g.numel() != k or dg.numel() != k or dv.shape != v.shape:
        raise ValueError("w2v_weightnorm_bwd: operand sizes do not match v (C, cg, k)")
    with _Timed("w2v_weightnorm_bwd_kernel", 0.0, [(C * cg, k)]):
        check(load().mmf_w2v_weightnorm_bwd(dw.data_ptr(), g.data_ptr(), v.data_ptr(), dg.data_ptr(), dv.data_ptr(), C, cg, k,
                                            int(bool(overwrite_v)), stream_ptr()))


# ---- DeBERTa kernels (csrc/deberta.hip) ------------------------------------------------------------------------
def _deberta_mask(mask, numel: int):
    """-> (pointer | None, mask_kind): an f32 mask as it is, a bool / uint8 one as bytes"""
    import torch
    if mask is None:
        return None, 0
    if not mask.is_cuda:
        raise RuntimeError("deberta kernels run on the GPU only (no CPU fallback)")
    if mask.dtype not in (torch.float32, torch.uint8, torch.bool) or not mask.is_contiguous() or mask.numel() != numel:
        raise ValueError("deberta: the mask must be a contiguous float32 / uint8 / bool tensor with one value per token")
    return mask.data_ptr(), 1 if mask.dtype == torch.float32 else 2


def deberta_embed(out, table, gamma, beta, eps: float, ids=None, embeds=None, mask=None) -> None:
    """out (rows, d) bf16 = LayerNorm(table[ids] | embeds) * mask: ids int64 (rows,), table f32 (vocab, d) or embeds f32 (rows, d)"""
    import torch
    _w2v_bf16(out)
    _w2v_f32(gamma, beta)
    if (ids is None) == (embeds is None):
        raise ValueError("deberta_embed: exactly one of ids / embeds")
    rows, d = out.shape
    if ids is not None:
        _w2v_f32(table)
        if not ids.is_cuda:
            raise RuntimeError("deberta kernels run on the GPU only (no CPU fallback)")
        if ids.dtype != torch.int64 or not ids.is_contiguous() or ids.numel() != rows or table.dim() != 2 or table.shape[1] != d:
            raise ValueError("deberta_embed: ids must be contiguous int64, one per output row, and table (vocab, d)")
    else:
        _w2v_f32(embeds)
        if embeds.numel() != rows * d:
            raise ValueError("deberta_embed: embeds must hold (rows, d) values")
    if not out.is_contiguous() or gamma.numel() != d or beta.numel() != d:
        raise ValueError("deberta_embed: out must be contiguous and gamma / beta one value per column")
    mp, kind = _deberta_mask(mask, rows)
    with _Timed("deberta_embed_kernel", 0.0, [(rows, d)]):
        check(load().mmf_deberta_embed(ids.data_ptr() if ids is not None else None, embeds.data_ptr() if embeds is not None else None,
                                       table.data_ptr() if ids is not None else None, gamma.data_ptr(), beta.data_ptr(), eps, mp, kind,
                                       out.data_ptr(), rows, d, table.shape[0] if ids is not None else 0, stream_ptr()))


def _deberta_attn_args(who: str, qkv, posq, posk, idx, out, n: int, H: int, T: int, S: int, head_dim: int) -> None:
    import torch
    _w2v_bf16(qkv, posq, posk, out)
    d = H * head_dim
    if not idx.is_cuda or idx.dtype != torch.int32 or not idx.is_contiguous() or idx.numel() != 2 * T - 1:
        raise ValueError(f"{who}: idx must be a contiguous int32 GPU tensor of 2 T - 1 values")
    if (qkv.numel() < n * T * 3 * d or out.numel() < n * T * d or not qkv.is_contiguous() or not out.is_contiguous()
            or tuple(posq.shape) != (2 * S, d) or tuple(posk.shape) != (2 * S, d) or posq.stride() != posk.stride() or posq.stride(1) != 1):
        raise ValueError(f"{who}: operand sizes do not match n, H, T, S")


def deberta_attn_fwd(qkv, posq, posk, idx, mask, out, n: int, H: int, T: int, S: int, scale: float, head_dim: int = 64, lse=None,
                     drop=None) -> None:
    """out (n T, H 64) bf16 = disentangled attention of the fused qkv rows (n T, 3 H 64); posq / posk (2S, H 64) bf16 views with a
    common row stride; idx int32 (2T - 1,) (include/mmfusion.h states its contract); mask (n, T) or None.  With ``lse`` (f32, n H T
    values) the launch also writes the rows' log-sum-exp for ``deberta_attn_bwd``; ``out`` is the same bits either way.
    ``drop`` = (p, state, site, item0): training-mode dropout of the probabilities (``mmf_deberta_attn_fwd_drop``); lse stays the
    undropped one"""
    _deberta_attn_args("deberta_attn_fwd", qkv, posq, posk, idx, out, n, H, T, S, head_dim)
    if lse is not None:
        _w2v_f32(lse)
        if lse.numel() < n * H * T:
            raise ValueError("deberta_attn_fwd: lse must hold n H T values")
    mp, kind = _deberta_mask(mask, n * T)
    with _Timed(f"deberta_attn_fwd_kernel<{head_dim}>", 12.0 * n * H * T * T * head_dim, [(T, T)]):
        if drop is not None:
            check(load().mmf_deberta_attn_fwd_drop(qkv.data_ptr(), posq.data_ptr(), posk.data_ptr(), posq.stride(0), idx.data_ptr(), mp, kind,
                                                   out.data_ptr(), None if lse is None else lse.data_ptr(), n, H, T, S, head_dim, scale,
                                                   *_drop_args("deberta_attn_fwd", drop), stream_ptr()))
        elif lse is None:
            check(load().mmf_deberta_attn_fwd(qkv.data_ptr(), posq.data_ptr(), posk.data_ptr(), posq.stride(0), idx.data_ptr(), mp, kind,
                                              out.data_ptr(), n, H, T, S, head_dim, scale, stream_ptr()))
        else:
            check(load().mmf_deberta_attn_fwd_lse(qkv.data_ptr(), posq.data_ptr(), posk.data_ptr(), posq.stride(0), idx.data_ptr(), mp, kind,
                                                  out.data_ptr(), lse.data_ptr(), n, H, T, S, head_dim, scale, stream_ptr()))


def _deberta_attn_bwd_args(who: str, qkv, posq, posk, idx, out, lse, dout, delta_ws, dqkv, n: int, H: int, T: int, S: int, head_dim: int) -> None:
    """the operand checks of ``deberta_attn_bwd`` and ``deberta_attn_bwd_pos`` (``who``: the one that was called)"""
    _deberta_attn_args(who, qkv, posq, posk, idx, out, n, H, T, S, head_dim)
    _w2v_bf16(dout, dqkv)
    _w2v_f32(lse, delta_ws)
    d = H * head_dim
    if (dout.numel() < n * T * d or dqkv.numel() < n * T * 3 * d or not dout.is_contiguous() or not dqkv.is_contiguous()
            or lse.numel() < n * H * T or delta_ws.numel() < n * H * T):
        raise ValueError(f"{who}: operand sizes do not match n, H, T")


def deberta_attn_bwd(qkv, posq, posk, idx, mask, out, lse, dout, delta_ws, dqkv, n: int, H: int, T: int, S: int, scale: float,
                     head_dim: int = 64, drop=None) -> None:
    """dqkv (n T, 3 H 64) bf16 <- the gradient of the fused qkv rows for the gradient ``dout`` (n T, H 64) of ``out``; ``out`` / ``lse``
    as ``deberta_attn_fwd(..., lse=lse)`` wrote them; ``delta_ws`` f32 scratch of n H T values.  Every row of dqkv is written.
    ``drop``: the forward's (p, state, site, item0), the mask drawn again (``mmf_deberta_attn_bwd_drop``)."""
    _deberta_attn_bwd_args("deberta_attn_bwd", qkv, posq, posk, idx, out, lse, dout, delta_ws, dqkv, n, H, T, S, head_dim)
    mp, kind = _deberta_mask(mask, n * T)
    # the forward's three score products again, dP, and two products (content + position) for each of dQ and dK, and dV
    with _Timed(f"deberta_attn_bwd_kernels<{head_dim}>", 22.0 * n * H * T * T * head_dim, [(T, T)]):
        args = (qkv.data_ptr(), posq.data_ptr(), posk.data_ptr(), posq.stride(0), idx.data_ptr(), mp, kind, out.data_ptr(), lse.data_ptr(),
                dout.data_ptr(), delta_ws.data_ptr(), dqkv.data_ptr(), n, H, T, S, head_dim, scale)
        if drop is not None:
            check(load().mmf_deberta_attn_bwd_drop(*args, *_drop_args("deberta_attn_bwd", drop), stream_ptr()))
        else:
            check(load().mmf_deberta_attn_bwd(*args, stream_ptr()))


def deberta_attn_bwd_pos_workspace_bytes(n: int, H: int, T: int, S: int) -> int:
    return int(load().mmf_deberta_attn_bwd_pos_workspace_bytes(n, H, T, S))


def deberta_attn_bwd_pos(qkv, posq, posk, idx, mask, out, lse, dout, delta_ws, dqkv, dposq, dposk, workspace, n: int, H: int, T: int,
                         S: int, scale: float, head_dim: int = 64, drop=None) -> None:
    """``deberta_attn_bwd`` (the same dqkv bits) that also ADDS the gradients of the position tables into ``dposq`` / ``dposk``: f32
    (2S, H 64) views with a common row stride, zeroed by the caller before the first chunk; ``workspace``: a contiguous f32 / uint8
    tensor of at least ``deberta_attn_bwd_pos_workspace_bytes(n, H, T, S)`` bytes (it need not be initialised).  ``drop`` as
    ``deberta_attn_bwd``'s (``mmf_deberta_attn_bwd_pos_drop``)."""
    import torch
    _deberta_attn_bwd_args("deberta_attn_bwd_pos", qkv, posq, posk, idx, out, lse, dout, delta_ws, dqkv, n, H, T, S, head_dim)
    d = H * head_dim
    if (not dposq.is_cuda or not dposk.is_cuda or dposq.dtype != torch.float32 or dposk.dtype != torch.float32
            or tuple(dposq.shape) != (2 * S, d) or tuple(dposk.shape) != (2 * S, d) or dposq.stride() != dposk.stride() or dposq.stride(1) != 1
            or not workspace.is_cuda or not workspace.is_contiguous()):
        raise ValueError("deberta_attn_bwd_pos: dposq / dposk must be (2S, H 64) f32 views with a common row stride, workspace contiguous")
    mp, kind = _deberta_mask(mask, n * T)
    # deberta_attn_bwd's products plus the two table contractions (2S x 64 x the tokens, per head)
    with _Timed(f"deberta_attn_bwd_pos_kernels<{head_dim}>", 22.0 * n * H * T * T * head_dim, [(T, T)]):
        args = (qkv.data_ptr(), posq.data_ptr(), posk.data_ptr(), posq.stride(0), idx.data_ptr(), mp, kind, out.data_ptr(), lse.data_ptr(),
                dout.data_ptr(), delta_ws.data_ptr(), dqkv.data_ptr(), n, H, T, S, head_dim, scale, dposq.data_ptr(), dposk.data_ptr(),
                dposq.stride(0), workspace.data_ptr(), workspace.numel() * workspace.element_size())
        if drop is not None:
            check(load().mmf_deberta_attn_bwd_pos_drop(*args, *_drop_args("deberta_attn_bwd_pos", drop), stream_ptr()))
        else:
            check(load().mmf_deberta_attn_bwd_pos(*args, stream_ptr()))


def hidden_dropout(y, out, items: int, drop, resid=None) -> None:
    """Hidden dropout of ``items`` items (``mmf_hidden_dropout``; DeBERTa's and Wav2Vec2's hidden sites): out = keep ? y c : 0 (+ ``resid``), element e of item g keyed by
    sub-stream item0 + g and index e of ``drop`` = (p, state, site, item0).  bf16: y, out and the optional ``resid`` are contiguous
    bf16 of one size, one f32 multiply-add and one rounding.  f32: y and out contiguous f32, no ``resid``.  ``out`` may be ``y``."""
    import torch
    f32 = y.dtype == torch.float32
    (_w2v_f32 if f32 else _w2v_bf16)(y, out)
    if resid is not None:
        if f32:
            raise ValueError("hidden_dropout: the f32 form takes no residual")
        _w2v_bf16(resid)
    ts = [y, out] + ([resid] if resid is not None else [])
    if items <= 0 or y.numel() % items or any(t.numel() != y.numel() or not t.is_contiguous() for t in ts):
        raise ValueError("hidden_dropout: y, out and resid must be contiguous, of one size that the items divide")
    with _Timed("hidden_dropout_kernel", 0.0, [(items, y.numel() // items)]):
        check(load().mmf_hidden_dropout(y.data_ptr(), None if resid is None else resid.data_ptr(), out.data_ptr(), int(f32), items,
                                        y.numel() // items, *_drop_args("hidden_dropout", drop), stream_ptr()))


def bias_gelu_drop_to(h, bias, g, items: int, drop) -> None:
    """g <- keep ? gelu(h + bias) c : 0 (``mmf_bias_gelu_drop_bf16_to``): ``bias_gelu_to`` with dropout of the GELU's output; the rows
    are ``items`` items, element (t, j) of item i keyed by sub-stream item0 + i and index t cols + j of ``drop`` = (p, state, site,
    item0).  ``g`` may be ``h``"""
    _w2v_bf16(h, g)
    _w2v_f32(bias)
    _gelu_blocks("bias_gelu_drop_to", bias, h, g)
    with _Timed("bias_gelu_drop_kernel", 0.0, [tuple(h.shape)]):
        check(load().mmf_bias_gelu_drop_bf16_to(h.data_ptr(), None if bias is None else bias.data_ptr(), g.data_ptr(), h.shape[0], h.shape[1],
                                                h.stride(0), int(items), *_drop_args("bias_gelu_drop_to", drop), stream_ptr()))


def bias_gelu_drop_bwd(dg, h, bias, dh, items: int, drop) -> None:
    """dh <- keep ? dg c gelu'(h + bias) : 0 (``mmf_bias_gelu_drop_bwd_bf16``), the mask of ``bias_gelu_drop_to`` drawn again"""
    _w2v_bf16(dg, h, dh)
    _w2v_f32(bias)
    _gelu_blocks("bias_gelu_drop_bwd", bias, dg, h, dh)
    with _Timed("bias_gelu_drop_bwd_kernel", 0.0, [tuple(h.shape)]):
        check(load().mmf_bias_gelu_drop_bwd_bf16(dg.data_ptr(), h.data_ptr(), None if bias is None else bias.data_ptr(), dh.data_ptr(), h.shape[0],
                                                 h.shape[1], h.stride(0), int(items), *_drop_args("bias_gelu_drop_bwd", drop), stream_ptr()))


def _w2v_starts(who: str, starts, items: int) -> int:
    import torch
    if not starts.is_cuda or starts.dtype != torch.int32 or starts.dim() != 2 or not starts.is_contiguous() or starts.shape[0] < items:
        raise ValueError(f"{who}: starts must be a contiguous int32 GPU tensor (clips, slots) of at least {items} clips")
    return starts.shape[1]


def w2v_mask_spans(starts, T: int, mask_prob: float, length: int, min_masks: int, state, site: int, item0: int = 0) -> None:
    """starts (N, S_max) int32 <- every clip's span starts of SpecAugment's time mask, -1 in unused slots (``mmf_w2v_mask_spans``;
    include/mmfusion.h states the draw)"""
    S = _w2v_starts("w2v_mask_spans", starts, 1)
    _, sp, site, item0 = _drop_args("w2v_mask_spans", (0.0, state, site, item0))
    with _Timed("w2v_mask_spans_kernel", 0.0, [tuple(starts.shape)]):
        check(load().mmf_w2v_mask_spans(starts.data_ptr(), starts.shape[0], S, int(T), float(mask_prob), int(length), int(min_masks), sp, site,
                                        item0, stream_ptr()))


def w2v_mask_drop(x, out, items: int, T: int, length: int, drop, starts=None, embed=None) -> None:
    """out <- rows inside a span of ``starts`` (the rows of the ``items`` clips; None: no masking) = bf16(``embed``) (f32 (d,); None:
    zeros, the gradient form), every other row keep ? x c : 0 under ``drop`` = (p, state, site, item0) (``mmf_w2v_mask_drop``).
    x, out: contiguous bf16 (items T, d); ``out`` may be ``x``"""
    _w2v_bf16(x, out)
    if x.dim() != 2 or x.shape != out.shape or x.shape[0] != items * T or not x.is_contiguous() or not out.is_contiguous():
        raise ValueError("w2v_mask_drop: x and out must be contiguous (items T, d)")
    S = _w2v_starts("w2v_mask_drop", starts, items) if starts is not None else 0
    if embed is not None:
        _w2v_f32(embed)
        if embed.numel() != x.shape[1] or not embed.is_contiguous():
            raise ValueError("w2v_mask_drop: embed must be contiguous f32 (d,)")
    with _Timed("w2v_mask_drop_kernel", 0.0, [tuple(x.shape)]):
        check(load().mmf_w2v_mask_drop(x.data_ptr(), None if embed is None else embed.data_ptr(), None if starts is None else starts.data_ptr(),
                                       out.data_ptr(), int(items), int(T), x.shape[1], S, int(length), *_drop_args("w2v_mask_drop", drop),
                                       stream_ptr()))


def w2v_mask_embed_grad(dx, starts, partial, items: int, T: int, length: int) -> None:
    """partial (slabs, d) f32 <- per slab of rows the sum of the rows of ``dx`` (items T, d) bf16 that lie inside a span
    (``mmf_w2v_mask_embed_grad``); ``sum_slabs`` finishes the mask embedding's gradient"""
    _w2v_bf16(dx)
    _w2v_f32(partial)
    S = _w2v_starts("w2v_mask_embed_grad", starts, items)
    if dx.dim() != 2 or dx.shape[0] != items * T or not dx.is_contiguous() or partial.dim() != 2 or partial.shape[1] != dx.shape[1] \
            or not partial.is_contiguous():
        raise ValueError("w2v_mask_embed_grad: dx must be contiguous (items T, d) and partial contiguous f32 (slabs, d)")
    with _Timed("w2v_mask_embed_grad_kernel", 0.0, [tuple(dx.shape)]):
        check(load().mmf_w2v_mask_embed_grad(dx.data_ptr(), starts.data_ptr(), partial.data_ptr(), int(items), int(T), dx.shape[1], S, int(length),
                                             partial.shape[0], stream_ptr()))


def deberta_embed_bwd(embeds, gamma, eps: float, mask, dout, d_embeds) -> None:
    """d_embeds (rows, d) f32 <- mask * the LayerNorm input gradient of ``dout`` (rows, d) bf16, the gradient of
    ``deberta_embed(out, ..., embeds=embeds)``'s output"""
    _w2v_f32(embeds, gamma, d_embeds)
    _w2v_bf16(dout)
    rows, d = dout.shape
    if embeds.numel() != rows * d or d_embeds.numel() != rows * d or gamma.numel() != d or not dout.is_contiguous() or not d_embeds.is_contiguous():
        raise ValueError("deberta_embed_bwd: embeds / d_embeds must hold (rows, d) values and gamma one value per column")
    mp, kind = _deberta_mask(mask, rows)
    with _Timed("deberta_embed_bwd_kernel", 0.0, [(rows, d)]):
        check(load().mmf_deberta_embed_bwd(embeds.data_ptr(), gamma.data_ptr(), eps, mp, kind, dout.data_ptr(), d_embeds.data_ptr(), rows, d,
                                           stream_ptr()))


def _deberta_ids(who: str, ids, rows: int) -> None:
    import torch
    if not ids.is_cuda:
        raise RuntimeError("deberta kernels run on the GPU only (no CPU fallback)")
    if ids.dtype != torch.int64 or not ids.is_contiguous() or ids.numel() != rows:
        raise ValueError(f"{who}: ids must be contiguous int64, one per row")


def deberta_embed_bwd_params_workspace_bytes(rows: int, d: int) -> int:
    return int(load().mmf_deberta_embed_bwd_params_workspace_bytes(rows, d))


def deberta_embed_bwd_params(gamma, eps: float, mask, dout, d_rows, dgamma, dbeta, workspace, ids=None, table=None, embeds=None,
                             accumulate: bool = False) -> None:
    """The backward of ``deberta_embed`` on the route it took (``ids`` int64 (rows,) with ``table`` f32 (vocab, d), or ``embeds`` f32
    (rows, d)) for the gradient ``dout`` (rows, d) bf16 of its output: d_rows (rows, d) f32 <- (``accumulate``: +=) the source
    rows' gradient (``deberta_embed_bwd``'s bits on the embeds route), and the LayerNorm's dgamma / dbeta (d,) f32 += theirs.
    ``workspace``: a contiguous f32 tensor of at least ``deberta_embed_bwd_params_workspace_bytes(rows, d)`` bytes (it need not be
    initialised)."""
    _w2v_f32(gamma, d_rows, dgamma, dbeta, workspace)
    _w2v_bf16(dout)
    if (ids is None) == (embeds is None):
        raise ValueError("deberta_embed_bwd_params: exactly one of ids / embeds")
    rows, d = dout.shape
    if ids is not None:
        _deberta_ids("deberta_embed_bwd_params", ids, rows)
        _w2v_f32(table)
        if table.dim() != 2 or table.shape[1] != d:
            raise ValueError("deberta_embed_bwd_params: table must be (vocab, d)")
    else:
        _w2v_f32(embeds)
        if embeds.numel() != rows * d:
            raise ValueError("deberta_embed_bwd_params: embeds must hold (rows, d) values")
    if (d_rows.numel() != rows * d or gamma.numel() != d or dgamma.numel() != d or dbeta.numel() != d or not dout.is_contiguous()
            or not d_rows.is_contiguous() or not workspace.is_contiguous()):
        raise ValueError("deberta_embed_bwd_params: d_rows must hold (rows, d) values, gamma / dgamma / dbeta one value per column")
    mp, kind = _deberta_mask(mask, rows)
    with _Timed("deberta_embed_bwd_params_kernels", 0.0, [(rows, d)]):
        check(load().mmf_deberta_embed_bwd_params(ids.data_ptr() if ids is not None else None, embeds.data_ptr() if embeds is not None else None,
                                                  table.data_ptr() if ids is not None else None, table.shape[0] if ids is not None else 0,
                                                  gamma.data_ptr(), eps, mp, kind, dout.data_ptr(), d_rows.data_ptr(), int(bool(accumulate)),
                                                  dgamma.data_ptr(), dbeta.data_ptr(), workspace.data_ptr(),
                                                  workspace.numel() * workspace.element_size(), rows, d, stream_ptr()))


def embedding_scatter_add(ids, d_rows, dtable, mask=None) -> None:
    """dtable[clamp(ids[r])] += d_rows[r] over the rows whose ``mask`` is not 0: ids int64 (rows,), d_rows f32 (rows, d), dtable f32
    (vocab, d); occurrences of an id are added in ascending row order, without atomics"""
    _w2v_f32(d_rows, dtable)
    if d_rows.dim() != 2 or dtable.dim() != 2 or dtable.shape[1] != d_rows.shape[1] or not d_rows.is_contiguous() or not dtable.is_contiguous():
        raise ValueError("embedding_scatter_add: d_rows (rows, d) and dtable (vocab, d) must be contiguous with one width")
    rows, d = d_rows.shape
    _deberta_ids("embedding_scatter_add", ids, rows)
    mp, kind = _deberta_mask(mask, rows)
    with _Timed("embedding_scatter_add_kernel", 0.0, [(rows, d)]):
        check(load().mmf_embedding_scatter_add_f32(ids.data_ptr(), mp, kind, d_rows.data_ptr(), dtable.data_ptr(), rows, d, dtable.shape[0],
                                                   stream_ptr()))


# ---- input preparation (csrc/prep.hip); tensors, not pointers: the shapes are checked here ------------------------
def _prep_f32(who: str, *ts) -> None:
    import torch
    for t in ts:
        if not t.is_cuda:
            raise RuntimeError(f"{who} runs on the GPU only (no CPU fallback)")
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"{who}: expected a contiguous float32 tensor, got {tuple(t.shape)} {t.dtype}")


def _prep_arg(t, who: str, dtype, numel: int, dev):
    """-> the pointer of an optional per-frame / per-clip array (None: null), checked"""
    if t is None:
        return None
    if t.device != dev or t.dtype != dtype or not t.is_contiguous() or t.numel() != numel:
        raise ValueError(f"{who} must be a contiguous {str(dtype).rpartition('.')[2]} tensor of {numel} values on {dev}, "
                         f"got {tuple(t.shape)} {t.dtype} on {t.device}")
    return t.data_ptr()


def video_prepare(frames, out, H: int, W: int, P: Optional[int] = None, bgr: bool = False, live=None, brightness=None,
                  flip=None) -> None:
    """frames (N, Hs, Ws, 3) uint8 contiguous -> out: (N, 3, H, W) f32, or with ``P`` the (N * (H/P) * (W/P), 3*P*P) bf16 patch
    matrix of ``vit_patchify``; live / flip uint8 (N,), brightness f32 (N,), all optional"""
    import torch
    if not frames.is_cuda or not out.is_cuda:
        raise RuntimeError("video_prepare runs on the GPU only (no CPU fallback)")
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 or not frames.is_contiguous():
        raise ValueError(f"video_prepare: frames must be contiguous uint8 (N, Hs, Ws, 3), got {tuple(frames.shape)} {frames.dtype}")
    N, Hs, Ws, _ = frames.shape
    if out.dtype != (torch.float32 if P is None else torch.bfloat16) or out.numel() != N * 3 * H * W or not out.is_contiguous():
        raise ValueError("video_prepare: out does not hold N x 3 x H x W contiguous f32 (pixels) / bf16 (patches) elements")
    dev = frames.device
    lp, fp = _prep_arg(live, "video_prepare: live", torch.uint8, N, dev), _prep_arg(flip, "video_prepare: flip", torch.uint8, N, dev)
    bp = _prep_arg(brightness, "video_prepare: brightness", torch.float32, N, dev)
    nbytes = N * (Hs * Ws * 3 + 3 * H * W * (4 if P is None else 2))
    with _Timed("video_prepare_kernel<%s>" % ("false" if P is None else "true"), 0.0, [(N, nbytes // N)]):
        if P is None:
            check(load().mmf_video_prepare(frames.data_ptr(), lp, bp, fp, out.data_ptr(), N, Hs, Ws, H, W, int(bgr), stream_ptr()))
        else:
            check(load().mmf_video_prepare_patches(frames.data_ptr(), lp, bp, fp, out.data_ptr(), N, Hs, Ws, H, W, P, int(bgr),
                                                   stream_ptr()))


def audio_resample(wave, lengths, table, out, orig: int, new: int, width: int) -> None:
    """wave (B, C, Ls) f32 -> out (B, L) f32: mono mean, resampling by new / orig against ``table`` (new, 2 width + orig) f32
    (None when orig == new), zeros past each clip's resampled length; lengths int32 (B,) or None"""
    import torch
    _prep_f32("audio_resample", wave, out)
    if wave.dim() != 3 or out.dim() != 2 or out.shape[0] != wave.shape[0]:
        raise ValueError(f"audio_resample: wave must be (B, C, Ls) and out (B, L), got {tuple(wave.shape)} and {tuple(out.shape)}")
    B, Cn, Ls = wave.shape
    if table is not None:
        _prep_f32("audio_resample", table)
    lp = _prep_arg(lengths, "audio_resample: lengths", torch.int32, B, wave.device)
    taps = 2 * width if table is not None else 1
    # (two kernels behind one entry point: audio_resample_tile_kernel where the phases fit LDS, audio_resample_kernel otherwise)
    with _Timed("audio_resample_kernels", 2.0 * out.numel() * taps, [(B, Cn * Ls * 4 + out.shape[1] * 4)]):
        check(load().mmf_audio_resample(wave.data_ptr(), lp, table.data_ptr() if table is not None else None,
                                        table.numel() if table is not None else 0, out.data_ptr(), B, Cn, Ls, out.shape[1], orig, new,
                                        width, stream_ptr()))


def audio_augment(x, out, noise_on, stretch_len, rng_state_ptr: Optional[int], site: int) -> None:
    """x (B, L) f32 -> out (B, L) f32: additive noise where noise_on (uint8 (B,)), then the time stretch to stretch_len
    (int32 (B,), L: off); either may be None"""
    import torch
    _prep_f32("audio_augment", x, out)
    if x.dim() != 2 or out.shape != x.shape or out.data_ptr() == x.data_ptr():
        raise ValueError("audio_augment: x and out must be two (B, L) tensors")
    B, L = x.shape
    np_ = _prep_arg(noise_on, "audio_augment: noise_on", torch.uint8, B, x.device)
    sp = _prep_arg(stretch_len, "audio_augment: stretch_len", torch.int32, B, x.device)
    with _Timed("audio_augment_kernel", 0.0, [(B, L * 8)]):
        check(load().mmf_audio_augment(x.data_ptr(), out.data_ptr(), np_, sp, rng_state_ptr, site, B, L, stream_ptr()))


# ---- Whisper's front end (csrc/whisper.hip) -------------------------------------------------------------------------------
WHISPER_DFT_COLS = 224           # MMF_WHISPER_DFT_COLS of include/mmfusion.h: the bins' columns of each half of the DFT table


def whisper_logmel_scratch_bytes(N: int, n_samples: int, n_mels: int) -> int:
    return int(load().mmf_whisper_logmel_scratch_bytes(N, n_samples, n_mels))


def whisper_logmel(wave, window, dft, mel_fb, scratch, n_samples: int, features=None, out_window=None) -> None:
    """wave (N, L) f32 (rows may be strided) -> ``features`` (N, n_mels, Tm) f32 and / or ``out_window`` (N, Tm, Kw) bf16
    (``mmf_whisper_logmel``); ``window`` [400], ``dft`` (400, 2 WHISPER_DFT_COLS) and ``mel_fb`` (201, n_mels) are the host's f32
    tables, ``scratch`` any contiguous buffer of ``whisper_logmel_scratch_bytes`` bytes"""
    import torch
    for t in (wave, window, dft, mel_fb, scratch, features, out_window):
        if t is not None and not t.is_cuda:
            raise RuntimeError("whisper_logmel runs on the GPU only (no CPU fallback)")
    if wave.dim() != 2 or wave.dtype != torch.float32 or wave.stride(1) != 1:
        raise ValueError(f"whisper_logmel: wave must be (N, L) f32 with contiguous rows, got {tuple(wave.shape)} {wave.dtype}")
    N, L = wave.shape
    Tm = n_samples // 160
    if mel_fb.dim() != 2 or mel_fb.shape[0] != 201 or window.numel() != 400 or dft.numel() != 400 * 2 * WHISPER_DFT_COLS or any(
            t.dtype != torch.float32 or not t.is_contiguous() for t in (window, dft, mel_fb)):
        raise ValueError("whisper_logmel: window [400], dft (400, 448) and mel_fb (201, n_mels) must be contiguous f32")
    n_mels, Kw = mel_fb.shape[1], 0
    if features is not None and (features.dtype != torch.float32 or tuple(features.shape) != (N, n_mels, Tm) or not features.is_contiguous()):
        raise ValueError(f"whisper_logmel: features must be contiguous f32 {(N, n_mels, Tm)}")
    if out_window is not None:
        if out_window.dtype != torch.bfloat16 or out_window.dim() != 3 or tuple(out_window.shape[:2]) != (N, Tm) or not out_window.is_contiguous():
            raise ValueError(f"whisper_logmel: out_window must be contiguous bf16 ({N}, {Tm}, Kw)")
        Kw = out_window.shape[2]
    if not scratch.is_contiguous():
        raise ValueError("whisper_logmel: scratch must be contiguous")
    with _Timed("whisper_logmel_kernels", 2.0 * N * Tm * 400 * 402, [(N, L)]):
        check(load().mmf_whisper_logmel(wave.data_ptr(), wave.stride(0) if N > 1 else L, window.data_ptr(), dft.data_ptr(), mel_fb.data_ptr(),
                                        None if features is None else features.data_ptr(),
                                        None if out_window is None else out_window.data_ptr(), scratch.data_ptr(),
                                        scratch.numel() * scratch.element_size(), N, L, n_samples, n_mels, Kw, stream_ptr()))


def whisper_feature_window(features, out_window) -> None:
    """features (N, n_mels, Tm) f32 -> out_window (N, Tm, Kw) bf16, ``whisper_logmel``'s window form of the same features"""
    import torch
    if not features.is_cuda or not out_window.is_cuda:
        raise RuntimeError("whisper_feature_window runs on the GPU only (no CPU fallback)")
    if features.dim() != 3 or features.dtype != torch.float32 or not features.is_contiguous():
        raise ValueError("whisper_feature_window: features must be contiguous f32 (N, n_mels, Tm)")
    N, n_mels, Tm = features.shape
    if out_window.dtype != torch.bfloat16 or out_window.dim() != 3 or tuple(out_window.shape[:2]) != (N, Tm) or not out_window.is_contiguous():
        raise ValueError(f"whisper_feature_window: out_window must be contiguous bf16 ({N}, {Tm}, Kw)")
    with _Timed("whisper_feature_window_kernel", 0.0, [(N * Tm, out_window.shape[2])]):
        check(load().mmf_whisper_feature_window(features.data_ptr(), out_window.data_ptr(), N, n_mels, Tm, out_window.shape[2], stream_ptr()))


def whisper_gelu_window(x, bias, out, N: int, T_in: int, C: int, k: int, s: int, pad: int) -> None:
    """x (N, T_in, C) bf16 raw convolution output, bias f32 [C] -> out (N, T_out, k * C) bf16: bias, exact GELU and the window form
    of a convolution with ``pad`` zero frames on both sides (``mmf_whisper_gelu_window``)"""
    _bf16_pair("whisper_gelu_window", x, out)
    T_out = (T_in + 2 * pad - k) // s + 1
    if x.numel() != N * T_in * C or out.numel() != N * T_out * k * C or bias.numel() != C:
        raise ValueError("whisper_gelu_window: operand sizes do not match N, T_in, C, k, s, pad")
    with _Timed("whisper_gelu_window_kernel", 0.0, [(N * T_out, k * C)]):
        check(load().mmf_whisper_gelu_window(x.data_ptr(), bias.data_ptr(), out.data_ptr(), N, T_in, C, k, s, pad, stream_ptr()))


def whisper_stem_out(x, bias, pos, out, T: int) -> None:
    """x (rows, d) bf16 raw convolution output of rows = n * T frames, bias f32 [d], pos f32 (T, d) -> out = bf16(gelu(x + bias) +
    pos[t]); out may be x (``mmf_whisper_stem_out``)"""
    _bf16_pair("whisper_stem_out", x, out)
    rows, d = x.shape
    if tuple(out.shape) != (rows, d) or bias.numel() != d or tuple(pos.shape) != (T, d) or not pos.is_contiguous():
        raise ValueError("whisper_stem_out: operand sizes do not match rows, T, d")
    with _Timed("whisper_stem_out_kernel", 0.0, [(rows, d)]):
        check(load().mmf_whisper_stem_out(x.data_ptr(), bias.data_ptr(), pos.data_ptr(), out.data_ptr(), rows, T, d, stream_ptr()))


def _bf16_pair(who: str, x, out) -> None:
    import torch
    if not x.is_cuda or not out.is_cuda:
        raise RuntimeError(f"{who} runs on the GPU only (no CPU fallback)")
    if x.dtype != torch.bfloat16 or out.dtype != torch.bfloat16 or not x.is_contiguous() or not out.is_contiguous():
        raise ValueError(f"{who}: x and out must be contiguous bf16")
