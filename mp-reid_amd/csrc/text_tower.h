// text_tower.h — what csrc/text_grad.hip (mpreid_text_backward) needs of the text tower in csrc/vit.hip: the workspace layout
// of mpreid_text_forward, its checks, and the launch sequence of its blocks.  The block driver itself (block_attention_part /
// block_mlp_part) stays in vit.hip; these are thin entry points over it, so the backward pass differentiates the activations
// the forward really produces.
#pragma once
#include "common.h"

// the workspace of mpreid_text_forward (byte offsets; every region 256-byte aligned)
struct TextLayout {
    int64_t M, Mpad;   // B * tokens, and M rounded up to the 256-row tiles of the big GEMM kernel
    size_t x, a, qkv, hbuf, y, total;
};
TextLayout text_layout(const mpreid_text_cfg *c, int B);
int text_check_cfg(const mpreid_text_cfg *c);                  // MPREID_ERR_ARG / MPREID_ERR_UNSUPPORTED with the error text set
int text_check_shape(int tokens, int width, int heads);

// x[m][:] = prompts[m][:] + pos[m % L][:]
int text_embed(const float *prompts, const float *pos, int64_t M, int L, int W, float *x, hipStream_t stream);

// One causal split-precision residual block over the M rows of x, in place: what mpreid_text_forward runs per layer.
// a: fp16 pairs [Mpad][2W]; qkv: fp32 [Mpad][3W]; hbuf: fp16 pairs [Mpad][8W].
int text_block(const mpreid_text_cfg *cfg, int B, const mpreid_vit_layer &ly, float *x, _Float16 *a, float *qkv, _Float16 *hbuf,
               int M, int Mpad, hipStream_t stream);

// The same launches up to FC1, for the backward sweep.  On entry x holds the block's input x_l; on return qkv holds
// q | k | v of ln_1(x_l) in fp32, x holds x_mid = x_l + out_proj(attention), and u [Mpad][4W] holds the FC1 pre-activation
// of ln_2(x_mid) in fp32 (FC1 with GE_S_BIAS_F32 in place of GE_S_BIAS_GELU).  FC2 is not run.
int text_block_recompute(const mpreid_text_cfg *cfg, int B, const mpreid_vit_layer &ly, float *x, _Float16 *a, float *qkv,
                         float *u, int M, int Mpad, hipStream_t stream);

// distance.hip: C[M][N] (row stride ldc) = A[M][K] x W[N][K]^T (+ bias[N]); exact fp32, k ascending, any M, N, K
int mpreid_gemm_f32_linear(const float *A, const float *Wt, int64_t M, int64_t N, int K, const float *bias, float *C,
                           int64_t ldc, int epi, hipStream_t stream);
enum { TEXT_F32_LIN = 2, TEXT_F32_LIN_RES = 4 };   // distance.hip: EPI_LIN, EPI_LIN_RES
