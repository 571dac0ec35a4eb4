"""ctypes binding of libmpreid_hip.so (include/mpreid.h).

There is no CPU fallback: if the library is missing, or a compute entry point is called without a
GPU, a RuntimeError is raised (SURVEY.md §8b "Errors").
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
#: MPREID_LIB points at another build of the same library (kernel A/B runs); there is no other fallback
LIB_PATH = os.environ.get("MPREID_LIB") or os.path.join(_HERE, "libmpreid_hip.so")

GEMM_F32_EXACT = 0
GEMM_F16_FAST = 1
GEMM_F16_SPLIT3 = 2
RERANK_AUTO, RERANK_DENSE, RERANK_SPARSE, RERANK_SPARSE_SPLIT3, RERANK_WIDE = 0, 1, 2, 3, 4
ERR_RETRY_DENSE = -5
ERR_ARG, ERR_WORKSPACE, ERR_UNSUPPORTED = -1, -2, -3
RANK_TOPK_MAX = 1024   # MPREID_RANK_TOPK_MAX
PAIR_BOUNDS_MAX = 4096   # MPREID_PAIR_BOUNDS_MAX

class RerankStats(C.Structure):
    _fields_ = [("n", C.c_int64), ("k1", C.c_int32), ("k2", C.c_int32), ("half_k1", C.c_int32),
                ("v_cap", C.c_int32), ("vqe_cap", C.c_int32), ("v_nnz", C.c_int64), ("vqe_nnz", C.c_int64),
                ("jaccard_pairs", C.c_int64), ("krecip_r_sum", C.c_int64), ("fallback_rows", C.c_int64),
                ("cand_total", C.c_int64), ("algo", C.c_int32), ("ms_gemm", C.c_float), ("ms_topk", C.c_float),
                ("ms_krecip", C.c_float), ("ms_qe", C.c_float), ("ms_csc", C.c_float),
                ("ms_jaccard", C.c_float), ("ms_total", C.c_float), ("ms_dq", C.c_float)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class VitCfg(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("img_h", "img_w", "patch", "stride", "h_res", "w_res", "width", "layers",
                                         "heads", "out_dim", "neck_after", "cls_only_last", "precision")]


class VitLayer(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("in_proj_w", "in_proj_b", "out_proj_w", "out_proj_b", "ln1_g", "ln1_b",
                                          "ln2_g", "ln2_b", "fc_w", "fc_b", "proj_w", "proj_b")] + \
               [(k, C.c_float) for k in ("in_proj_s", "out_proj_s", "fc_s", "proj_s")] + \
               [(k, C.c_void_p) for k in ("in_proj_c", "fc_c")]


class VitWeights(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("conv_w", "class_emb", "pos_emb", "ln_pre_g", "ln_pre_b", "ln_post_g",
                                          "ln_post_b", "proj", "bn_scale", "bn_shift", "bn_proj_scale",
                                          "bn_proj_shift")] + [("layers", C.POINTER(VitLayer)), ("conv_s", C.c_float)]


MOE_MAX_EXPERTS, MOE_MAX_TOPK = 64, 8   # MPREID_MOE_MAX_EXPERTS, MPREID_MOE_MAX_TOPK


class MoeLayer(C.Structure):
    """mpreid_moe_layer: one MoE block; fc_s / proj_s are DEVICE arrays [E]"""
    _fields_ = [(k, C.c_void_p) for k in ("gate_w", "fc_w", "fc_b", "proj_w", "proj_b", "fc_s", "proj_s")]


class MoeLayerT(C.Structure):
    """mpreid_moe_layer_t: per expert the fp32 transpose of the checkpoint's matrices, fc_t [E][w][4w], proj_t [E][4w][w]"""
    _fields_ = [(k, C.c_void_p) for k in ("fc_t", "proj_t")]


class MoeExpertGrads(C.Structure):
    """mpreid_moe_expert_grads: the expert matrices' own gradients (not implemented: every member NULL)"""
    _fields_ = [(k, C.c_void_p) for k in ("fc_w", "fc_b", "proj_w", "proj_b")]


class VitMoeT(C.Structure):
    """mpreid_vit_moe_t: a HOST array of moe_layers mpreid_moe_layer_t"""
    _fields_ = [("layers", C.POINTER(MoeLayerT))]


class VitMoe(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("num_experts", "top_k", "moe_layers")] + [("layers", C.POINTER(MoeLayer))]


TEXT_MAX_TOKENS = 128   # MPREID_TEXT_MAX_TOKENS
SUPCON_MAX_BATCH = 1024   # MPREID_SUPCON_MAX_BATCH
TRIPLET_MAX_BATCH = 1024  # MPREID_TRIPLET_MAX_BATCH


OPTIM_SGD, OPTIM_ADAM, OPTIM_ADAMW = 0, 1, 2   # MPREID_OPTIM_*
OPTIM_MAX_CLASSES, OPTIM_CHUNK, OPTIM_TENSORS_PER_LAUNCH = 8, 4096, 64
RESIZE_BILINEAR, RESIZE_BICUBIC = 0, 1   # MPREID_RESIZE_*
AUG_IMAGES_PER_LAUNCH = 64               # MPREID_AUG_IMAGES_PER_LAUNCH


class OptimEntry(C.Structure):
    """mpreid_optim_entry"""
    _fields_ = [(k, C.c_void_p) for k in ("param", "grad", "state1", "state2")] + [("n", C.c_int64), ("hyper", C.c_int32),
                                                                                    ("reserved_", C.c_int32)]


class OptimClass(C.Structure):
    """mpreid_optim_class"""
    _fields_ = [("lr", C.c_float), ("weight_decay", C.c_float)]


class AbsmaxEntry(C.Structure):
    """mpreid_absmax_entry"""
    _fields_ = [("src", C.c_void_p), ("n", C.c_int64)]


class TextCfg(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("tokens", "width", "layers", "heads", "out_dim")]


class TextWeights(C.Structure):
    """mpreid_text_weights: the layers are VitLayer entries in their split-mode layouts"""
    _fields_ = [(k, C.c_void_p) for k in ("pos_emb", "ln_final_g", "ln_final_b", "proj")] + [("layers", C.POINTER(VitLayer))]


class TextLayerT(C.Structure):
    """mpreid_text_layer_t: fp32 [in][out] copies of a block's four frozen matrices (the gradient GEMMs' operands)"""
    _fields_ = [(k, C.c_void_p) for k in ("in_proj_t", "out_proj_t", "fc_t", "proj_t")]


class TextWeightsT(C.Structure):
    """mpreid_text_weights_t"""
    _fields_ = [("proj_t", C.c_void_p), ("layers", C.POINTER(TextLayerT))]


class VitWeightsT(C.Structure):
    """mpreid_vit_weights_t: per block the fp32 [in][out] copies of its four matrices (TextLayerT's layout)"""
    _fields_ = [("layers", C.POINTER(TextLayerT))]


VIT_LAYER_GRADS = ("in_proj_w", "in_proj_b", "out_proj_w", "out_proj_b", "fc_w", "fc_b", "proj_w", "proj_b", "ln1_g", "ln1_b",
                   "ln2_g", "ln2_b")
VIT_TOWER_GRADS = ("conv_w", "class_emb", "pos_emb", "ln_pre_g", "ln_pre_b", "ln_post_g", "ln_post_b", "proj", "cv_emb")


class VitLayerGrads(C.Structure):
    """mpreid_vit_layer_grads: fp32 device pointers in torch layout, NULL = not wanted"""
    _fields_ = [(k, C.c_void_p) for k in VIT_LAYER_GRADS]


class VitGrads(C.Structure):
    """mpreid_vit_grads"""
    _fields_ = [(k, C.c_void_p) for k in VIT_TOWER_GRADS] + [("layers", C.POINTER(VitLayerGrads))]


class ImageIn(C.Structure):
    """mpreid_image_in: the image batch of every encoder forward; exactly one of the two pointers is non-NULL"""
    _fields_ = [("f32_dev", C.c_void_p), ("u8_hwc_dev", C.c_void_p), ("mean", C.c_float * 3), ("std", C.c_float * 3),
                ("view", C.c_int32)]


class Rn50Conv(C.Structure):
    _fields_ = [("w", C.c_void_p), ("bias", C.c_void_p), ("cin", C.c_int32), ("cout", C.c_int32),
                ("cout_pad", C.c_int32), ("taps", C.c_int32)]


class Rn50Block(C.Structure):
    _fields_ = [("conv1", Rn50Conv), ("conv2", Rn50Conv), ("conv3", Rn50Conv), ("down", Rn50Conv), ("stride", C.c_int32)]


class Rn50Cfg(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("img_h", "img_w", "width", "n_blocks", "heads", "out_dim")]


class Rn50Weights(C.Structure):
    _fields_ = [("stem1_w", C.c_void_p), ("stem1_b", C.c_void_p), ("stem2", Rn50Conv), ("stem3", Rn50Conv),
                ("blocks", C.POINTER(Rn50Block)), ("pos_emb", C.c_void_p), ("kt_w", C.c_void_p), ("v_w", C.c_void_p), ("v_b", C.c_void_p),
                ("q_w", C.c_void_p), ("q_b", C.c_void_p), ("c_w", C.c_void_p), ("c_b", C.c_void_p),
                ("bn_scale", C.c_void_p), ("bn_shift", C.c_void_p)]


class Rn50ConvF32(C.Structure):
    _fields_ = [("w", C.c_void_p), ("bias", C.c_void_p), ("cin", C.c_int32), ("cout", C.c_int32), ("taps", C.c_int32)]


class Rn50BlockF32(C.Structure):
    _fields_ = [("conv1", Rn50ConvF32), ("conv2", Rn50ConvF32), ("conv3", Rn50ConvF32), ("down", Rn50ConvF32),
                ("stride", C.c_int32)]


class Rn50WeightsF32(C.Structure):
    _fields_ = [("stem1_w", C.c_void_p), ("stem1_b", C.c_void_p), ("stem2", Rn50ConvF32), ("stem3", Rn50ConvF32),
                ("blocks", C.POINTER(Rn50BlockF32)), ("pos_emb", C.c_void_p), ("q_w", C.c_void_p), ("q_b", C.c_void_p),
                ("k_w", C.c_void_p), ("k_b", C.c_void_p), ("v_w", C.c_void_p), ("v_b", C.c_void_p), ("c_w", C.c_void_p),
                ("c_b", C.c_void_p), ("bn_scale", C.c_void_p), ("bn_shift", C.c_void_p)]


class Rn50ConvSplit(C.Structure):
    _fields_ = [("w", C.c_void_p), ("bias", C.c_void_p), ("cin", C.c_int32), ("cout", C.c_int32), ("taps", C.c_int32),
                ("kseg", C.c_int32), ("npad", C.c_int32), ("oscale", C.c_float)]


class Rn50BlockSplit(C.Structure):
    _fields_ = [("conv1", Rn50ConvSplit), ("conv2", Rn50ConvSplit), ("conv3", Rn50ConvSplit), ("down", Rn50ConvSplit),
                ("stride", C.c_int32)]


class Rn50WeightsSplit(C.Structure):
    _fields_ = [("f32", Rn50WeightsF32), ("blocks", C.POINTER(Rn50BlockSplit)), ("k", Rn50ConvSplit), ("v", Rn50ConvSplit),
                ("stem2", Rn50ConvSplit), ("stem3", Rn50ConvSplit)]


class ProfileEntry(C.Structure):
    _fields_ = [("epilogue", C.c_int32), ("n", C.c_int32), ("k", C.c_int32), ("m", C.c_int64),
                ("launches", C.c_int64), ("total_ms", C.c_double), ("flops_total", C.c_double)]


GEMM_EPILOGUE_NAMES = {0: "f32", 1: "qkv_bias_f16", 2: "bias_residual", 3: "fc_bias_quickgelu", 4: "patch_embed",
                       5: "euclid", 6: "cosine", 7: "conv1x1_bias_relu", 8: "conv1x1_bias_residual_relu", 9: "candidates",
                       10: "split_qkv_bias_f32", 11: "split_bias_residual", 12: "split_fc_bias_quickgelu",
                       13: "split_patch_embed"}
VIT_F16, VIT_SPLIT = 0, 1

#: mpreid_version() of the library this binding was written for: signatures change under unchanged names, so no other loads
VERSION = 102

vp, i64, i32, f32, f64, sz, P = C.c_void_p, C.c_int64, C.c_int, C.c_float, C.c_double, C.c_size_t, C.POINTER
_DIST = [vp, vp, i64, i64, i32, vp, i64, i32, vp, sz, vp]
_RERANK = [vp, vp, i64, i64, i32, i32, i32, f64, vp, i32, vp, i64, vp, sz, vp, P(RerankStats), i32]
_CSR = [vp, vp, vp, i64, i32, vp, vp, vp]
#: every function include/mpreid.h declares, once: name -> (restype, argtypes); load() applies it
PROTOTYPES = {
    "mpreid_version": (i32, []),
    "mpreid_is_ablation_build": (i32, []),
    "mpreid_last_error": (C.c_char_p, []),
    "mpreid_device_count": (i32, []),
    "mpreid_device_info": (i32, [C.c_char_p, i32, P(i32), P(sz)]),
    "mpreid_sqnorm_f32": (i32, [vp, i64, i32, vp, vp]),
    "mpreid_l2_normalize_f32": (i32, [vp, i64, i32, f32, vp, vp]),
    "mpreid_distance_workspace_bytes": (sz, [i64, i64, i32, i32]),
    "mpreid_euclidean_distance_f32": (i32, _DIST),
    "mpreid_cosine_similarity_f32": (i32, _DIST),
    "mpreid_rerank_workspace_bytes": (sz, [i64, i64, i32, i32, i32, i32]),
    "mpreid_rerank_f32": (i32, _RERANK),
    "mpreid_rerank_debug_copy": (i32, [vp, i64, i64, i32, i32, i32, i32, vp, vp, vp, vp]),
    "mpreid_rerank_workspace_bytes_ex": (sz, [i64, i64, i32, i32, i32, i32, i32]),
    "mpreid_rerank_fits": (i32, [i64, i64, i32, i32, i32, i32, i32]),
    "mpreid_rerank_f32_ex": (i32, _RERANK + [i32]),
    "mpreid_rerank_debug_copy_ex": (i32, [vp, i64, i64, i32, i32, i32, i32, vp, vp, vp, vp, i32]),
    "mpreid_eval_rank_positions": (i32, [vp, i64, i32, i32, vp, vp, i32, vp, vp, vp]),
    "mpreid_eval_rank_positions_cam": (i32, [vp, i64, i32, i32, vp, vp, vp, vp, i32, vp, vp, vp]),
    "mpreid_eval_rank_positions_splits": (i32, [vp, i64, i64, i64, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, i32, vp, vp, vp]),
    "mpreid_rank_topk": (i32, [vp, i64, i32, i32, i64, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp]),
    "mpreid_qe_aggregate_f32": (i32, [vp, i64, i32, i64, vp, vp, vp, i64, i32, f32, vp, i64, vp]),
    "mpreid_pair_bucket_counts": (i32, [vp, i64, i32, i32, vp, vp, vp, vp, vp, i32, i32, vp, vp]),
    "mpreid_rr_dist_rows": (i32, [vp, vp, i64, i32, i64, i64, vp, i64, vp, vp, i32, vp]),
    "mpreid_rr_vcap": (i32, [i64, i32]),
    "mpreid_rr_krecip_scratch_bytes": (sz, [i64]),
    "mpreid_rr_krecip": (i32, [vp, i64, i64, vp, vp, i32, i32, i64, i64, vp, vp, vp, vp, vp]),
    "mpreid_rr_sparse_workspace_bytes": (sz, [i64, i32, i64, i32]),
    "mpreid_rr_neighbours_sparse": (i32, [vp, vp, i64, i32, i64, i64, i32, vp, vp, vp, vp, sz, vp]),
    "mpreid_rr_krecip_sparse": (i32, [vp, vp, i64, i32, vp, vp, vp, i32, i32, i64, i64, vp, vp, vp, vp, vp]),
    "mpreid_rr_pack_rows": (i32, [vp, vp, vp, i64, i32, i32, vp, vp, vp]),
    "mpreid_rr_rowptr": (i32, [vp, i64, vp, vp]),
    "mpreid_rr_ell_to_csr": (i32, _CSR),
    "mpreid_rr_csr_to_ell": (i32, _CSR),
    "mpreid_rr_qe_count": (i32, [i64, vp, i32, i32, i64, i64, vp, vp, i32, vp, vp]),
    "mpreid_rr_qe_fill": (i32, [i64, vp, i32, i32, i64, i64, vp, vp, vp, i32, i32, vp, vp, vp, vp]),
    "mpreid_rr_jaccard": (i32, [i64, i64, i64, i64, vp, i64, vp, vp, vp, vp, i32, f64, vp, vp, vp, vp, vp, vp, i64, vp]),
    "mpreid_rr_jaccard_hist_bytes": (sz, [i64]),
    "mpreid_rr_csc_chunks": (i32, [i64, i64]),
    "mpreid_rr_csc_count": (i32, [i64, i64, vp, vp, i32, i64, i64, vp, vp, vp]),
    "mpreid_rr_csc_fill": (i32, [i64, i64, vp, vp, vp, i32, i64, i64, vp, vp, vp, vp, vp, vp]),
    "mpreid_rr_jaccard_indexed": (i32, [i64, i64, i64, i64, vp, i64, vp, vp, vp, vp, i32, f64, vp, vp, vp, vp, i64, vp]),
    # the encoders: (cfg, weights, image batch, B, [cv_emb,] out, workspace, workspace bytes, stream)
    "mpreid_vit_workspace_bytes": (sz, [P(VitCfg), i32]),
    "mpreid_vit_forward": (i32, [P(VitCfg), P(VitWeights), P(ImageIn), i32, vp, vp, vp, sz, vp]),
    "mpreid_vit_attention": (i32, [vp, i32, i32, i32, i32, i32, i32, vp, vp]),
    "mpreid_vit_workspace_bytes_f32": (sz, [P(VitCfg), i32]),
    "mpreid_vit_forward_f32": (i32, [P(VitCfg), P(VitWeights), P(ImageIn), i32, vp, vp, vp, sz, vp]),
    "mpreid_vit_attention_f32": (i32, [vp, i32, i32, i32, i32, vp, vp]),
    # the MoE image encoder: the forward takes the MoE description behind the weights; then the unit seams
    "mpreid_vit_workspace_bytes_moe": (sz, [P(VitCfg), P(VitMoe), i32]),
    "mpreid_vit_forward_moe": (i32, [P(VitCfg), P(VitWeights), P(VitMoe), P(ImageIn), i32, vp, vp, vp, sz, vp]),
    "mpreid_moe_workspace_bytes": (sz, [i64, i32, i32, i32]),
    "mpreid_moe_route": (i32, [vp, i64, i32, vp, vp, vp, i32, i32, vp, vp, vp, vp]),
    "mpreid_moe_mlp_split": (i32, [vp, i64, i32, vp, vp, i32, i32, P(MoeLayer), vp, vp, sz, vp]),
    # the gradient through one routed MLP (a_pairs, rows, width, sel, w, E, K, layer, layer_t, dy, d_a, d_w, accumulate, d_experts,
    # workspace, bytes, stream) and of the router (logits, rows, E, K, sel, w, d_w, aux_coef, d_logits, l_aux, workspace, bytes, stream)
    "mpreid_moe_grad_workspace_bytes": (sz, [i64, i32, i32, i32]),
    "mpreid_moe_mlp_backward": (i32, [vp, i64, i32, vp, vp, i32, i32, P(MoeLayer), P(MoeLayerT), vp, vp, vp, i32, P(MoeExpertGrads),
                                      vp, sz, vp]),
    "mpreid_moe_route_backward_workspace_bytes": (sz, [i64, i32]),
    "mpreid_moe_route_backward": (i32, [vp, i64, i32, i32, vp, vp, vp, f32, vp, vp, vp, sz, vp]),
    # the text tower: (cfg, weights, prompts, eot rows, B, out, workspace, workspace bytes, stream)
    "mpreid_text_workspace_bytes": (sz, [P(TextCfg), i32]),
    "mpreid_text_forward": (i32, [P(TextCfg), P(TextWeights), vp, vp, i32, vp, vp, sz, vp]),
    "mpreid_text_attention": (i32, [vp, i32, i32, i32, i32, vp, vp]),
    # its gradient with respect to the prompts: (cfg, weights, transposed fp32 weights, prompts, eot rows, grad_out, B,
    # grad_prompts, workspace, workspace bytes, stream)
    "mpreid_text_backward_workspace_bytes": (sz, [P(TextCfg), i32]),
    "mpreid_text_backward": (i32, [P(TextCfg), P(TextWeights), P(TextWeightsT), vp, vp, vp, i32, vp, vp, sz, vp]),
    "mpreid_text_attention_backward": (i32, [vp, vp, i32, i32, i32, i32, vp, vp]),
    "mpreid_layernorm_backward_f32": (i32, [vp, vp, vp, i64, i32, i32, vp, vp]),
    # three row kernels alone: (x, rows, width, gamma, beta, form, out, stream); (x, item_stride, row_of, tokens, batch, width,
    # out_dim, ln_g, ln_b, proj, bn_scale, bn_shift, bnp_scale, bnp_shift, y, out, out_stride, out_col, ln_to_out, stream);
    # (u, d, n, stream)
    "mpreid_layernorm_f32": (i32, [vp, i64, i32, vp, vp, i32, vp, vp]),
    "mpreid_tower_head_f32": (i32, [vp, i64, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp]),
    "mpreid_quickgelu_backward_f32": (i32, [vp, vp, i64, vp]),
    # the image tower's gradient: the training forward (cfg, weights, image batch, B, cv_emb, f_last, f, f_proj, workspace,
    # workspace bytes, stream) and the unmasked attention gradient (qkv, d_o, B, tokens, width, heads, d_qkv, workspace, bytes, stream)
    "mpreid_vit_forward_train": (i32, [P(VitCfg), P(VitWeights), P(ImageIn), i32, vp, vp, vp, vp, vp, sz, vp]),
    "mpreid_vit_attention_backward_workspace_bytes": (sz, [i32, i32, i32]),
    "mpreid_vit_attention_backward": (i32, [vp, vp, i32, i32, i32, i32, vp, vp, sz, vp]),
    # the sweep (cfg, weights, transposed weights, image batch, B, cv_emb, d_f_last, d_f, d_f_proj, grads, d_tokens, workspace,
    # workspace bytes, stream) and its two small kernels alone
    "mpreid_vit_backward_workspace_bytes": (sz, [P(VitCfg), i32]),
    "mpreid_vit_backward": (i32, [P(VitCfg), P(VitWeights), P(VitWeightsT), P(ImageIn), i32, vp, vp, vp, vp, P(VitGrads), vp, vp,
                                  sz, vp]),
    # the MoE tower: (cfg, weights, moe, image batch, B, cv_emb, f_last, f, f_proj, logits, l_aux, workspace, bytes, stream) and
    # (cfg, weights, transposed, moe, moe transposed, image batch, B, cv_emb, d_f_last, d_f, d_f_proj, aux_coef, grads, d_gate_w,
    # d_tokens, l_aux, workspace, bytes, stream)
    "mpreid_vit_forward_train_moe_workspace_bytes": (sz, [P(VitCfg), P(VitMoe), i32]),
    "mpreid_vit_forward_train_moe": (i32, [P(VitCfg), P(VitWeights), P(VitMoe), P(ImageIn), i32, vp, vp, vp, vp, vp, vp, vp, sz, vp]),
    "mpreid_vit_backward_moe_workspace_bytes": (sz, [P(VitCfg), P(VitMoe), i32]),
    "mpreid_vit_backward_moe": (i32, [P(VitCfg), P(VitWeights), P(VitWeightsT), P(VitMoe), P(VitMoeT), P(ImageIn), i32, vp, vp, vp,
                                      vp, f32, P(VitGrads), vp, vp, vp, vp, sz, vp]),
    "mpreid_transpose_pad_f32": (i32, [vp, i64, i32, vp, i64, vp]),
    "mpreid_colsum_workspace_bytes": (sz, [i64, i32]),
    "mpreid_colsum_f32": (i32, [vp, vp, i64, i32, vp, vp, vp, sz, vp]),
    # stage-1 prompt learning: the contrastive loss pair with its gradients, the context gradient, the Adam / AdamW step
    "mpreid_supcon_workspace_bytes": (sz, [i32, i32]),
    "mpreid_supcon_pair_f32": (i32, [vp, vp, vp, i32, i32, vp, vp, vp, vp, sz, vp]),
    "mpreid_supcon_f32": (i32, [vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, sz, vp]),
    "mpreid_rows_segment_sum_f32": (i32, [vp, vp, i32, i32, i32, i32, i32, i32, vp, vp]),
    "mpreid_adam_step_f32": (i32, [vp, vp, vp, vp, i64, i32, f32, f32, f32, f32, f32, i32, vp]),
    # stage-2 training: one optimizer step over a table of tensors, the largest finite |entry| per tensor of a table
    "mpreid_optim_step_launches": (i32, [i32]),
    "mpreid_optim_step_multi_f32": (i32, [P(OptimEntry), i32, P(OptimClass), i32, i32, i32, f32, f32, f32, f32, vp]),
    "mpreid_absmax_multi_workspace_bytes": (sz, [P(AbsmaxEntry), i32]),
    "mpreid_absmax_multi_f32": (i32, [P(AbsmaxEntry), i32, vp, vp, sz, vp]),
    # the stage-2 head: row cross-entropy, batch-hard triplet loss, BatchNorm1d in training mode, the linear products, the total
    "mpreid_xent_rows_f32": (i32, [vp, i64, vp, i32, i32, f32, f32, vp, vp, vp, vp, vp]),
    "mpreid_triplet_workspace_bytes": (sz, [i32, i32]),
    "mpreid_triplet_hard_f32": (i32, [vp, vp, i32, i32, f32, i32, f32, f32, vp, vp, vp, vp, vp, vp, vp, sz, vp]),
    "mpreid_bn1d_train_forward_f32": (i32, [vp, vp, vp, i32, i32, f32, f32, vp, vp, vp, vp, vp, vp]),
    "mpreid_bn1d_train_backward_f32": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp]),
    "mpreid_matmul_f32": (i32, [vp, i64, i64, vp, i64, i64, i32, i32, i32, vp, vp, i64, vp]),
    "mpreid_stage2_total_f32": (i32, [vp, i32, i32, i32, vp, vp]),
    "mpreid_tta_mean_f32": (i32, [vp, i32, i64, i32, i32, vp, vp]),
    "mpreid_resize_workspace_bytes": (sz, [i32, i32, i32]),
    "mpreid_resize_bilinear_u8": (i32, [vp, vp, vp, i32, i32, i32, i32, vp, vp, sz, vp]),
    # (src, offsets, hw, batch, max_in_h, out_h, out_w, filter, dst, workspace, bytes, stream); the training augmentation
    # (img_hwc, batch, H, W, pad, params HOST int32 [B][8], sample_id HOST int64 [B], seed, mean HOST [3], std HOST [3], out, stream)
    "mpreid_resize_u8": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, sz, vp]),
    "mpreid_train_augment_f32": (i32, [vp, i32, i32, i32, i32, vp, vp, C.c_uint64, vp, vp, vp, vp]),
    "mpreid_rn50_workspace_bytes": (sz, [P(Rn50Cfg), i32]),
    "mpreid_rn50_forward": (i32, [P(Rn50Cfg), P(Rn50Weights), P(ImageIn), i32, vp, vp, sz, vp]),
    "mpreid_rn50_workspace_bytes_f32": (sz, [P(Rn50Cfg), i32]),
    "mpreid_rn50_forward_f32": (i32, [P(Rn50Cfg), P(Rn50WeightsF32), P(ImageIn), i32, vp, vp, sz, vp]),
    "mpreid_rn50_workspace_bytes_split": (sz, [P(Rn50Cfg), i32]),
    "mpreid_rn50_forward_split": (i32, [P(Rn50Cfg), P(Rn50WeightsSplit), P(ImageIn), i32, vp, vp, sz, vp]),
    "mpreid_conv_f16_nhwc": (i32, [vp, i32, i32, i32, i32, vp, vp, i32, i32, i32, vp, i32, vp, vp, vp]),
    "mpreid_rn50_conv_split_layer": (i32, [P(Rn50ConvSplit), vp, i32, i32, vp, i32, i32, i32, i32, vp, vp, i32, vp, vp, vp]),
    "mpreid_gemm_f16_nt": (i32, [vp, vp, vp, i64, i64, i64, vp]),
    "mpreid_gemm_f16_nt_ex": (i32, [vp, vp, vp, vp, i64, i64, i64, i32, vp]),
    "mpreid_gemm_f16_split_nt": (i32, [vp, vp, vp, vp, i64, i64, i64, f32, i32, vp]),
    "mpreid_split_pack_f32": (i32, [vp, i64, i32, f32, vp, vp]),
    "mpreid_cast_f32_to_f16": (i32, [vp, vp, i64, vp]),
    "mpreid_profile_enable": (i32, [i32]),
    "mpreid_profile_reset": (i32, []),
    "mpreid_profile_query": (i32, [P(ProfileEntry), i32]),
}
#: every symbol include/mpreid.h declares (tests check the library exports all of them)
SYMBOLS = list(PROTOTYPES)

_lib = None


def load():
    """Load the library and declare prototypes.  Raises RuntimeError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    # torch bundles its own libamdhip64; it must be in the process BEFORE this library is dlopen-ed so that the
    # dynamic linker resolves our dependency to the same runtime.  Loaded the other way round the process holds
    # two HIP runtimes and the second one reports "no ROCm-capable device".
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python mp-reid_amd/mpreid/build.py` "
            "(or __graft_entry__.build()).  There is no CPU fallback for the HIP path.")
    L = C.CDLL(LIB_PATH)
    # MPREID_LIB may point at any build of the library.  One compiled with -DMPREID_ABLATION skips work on request (wrong
    # results by design): it must say so itself, and is refused unless the caller asked for exactly that.
    for name in ("mpreid_is_ablation_build", "mpreid_version"):
        if not hasattr(L, name):
            raise RuntimeError(f"{LIB_PATH} does not export {name}: a stale build; rebuild it")
        getattr(L, name).restype, getattr(L, name).argtypes = PROTOTYPES[name]
    if L.mpreid_is_ablation_build() and os.environ.get("MPREID_ALLOW_ABLATION") != "1":
        raise RuntimeError(f"{LIB_PATH} is a timing-ablation build (-DMPREID_ABLATION: wrong results by design); "
                           "set MPREID_ALLOW_ABLATION=1 to load it for a measurement")
    # the prototypes below are those of ONE version of include/mpreid.h: a library of another version may export the same
    # names with other arguments
    if L.mpreid_version() != VERSION:
        raise RuntimeError(f"{LIB_PATH} reports version {L.mpreid_version()}, this binding is written for {VERSION}: "
                           "a stale build; rebuild it")
    for name, (restype, argtypes) in PROTOTYPES.items():
        f = getattr(L, name)
        f.restype, f.argtypes = restype, argtypes
    _lib = L
    return L


def check(rc: int, what: str):
    if rc != 0:
        msg = load().mpreid_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"{what} failed (code {rc}): {msg}")


def require_gpu():
    """The compute entry points need a HIP device; fail loudly instead of falling back."""
    import torch
    load()
    if not torch.cuda.is_available():
        raise RuntimeError("mpreid HIP path needs an MI355X (no HIP device visible); there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
