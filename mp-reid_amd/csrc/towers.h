// towers.h — what the tower files share: csrc/vit.hip (the image towers, the residual-block driver, the head), csrc/text.hip
// (the text tower's forward) and csrc/text_grad.hip (mpreid_text_backward).  The block driver itself (block_attention_part /
// block_mlp_part) stays in vit.hip; text_block / text_block_recompute are thin entry points over it, so the backward pass
// differentiates the activations the forward really produces.
#pragma once
#include "common.h"

// the 256-byte aligned bump cursor of every workspace layout of the towers: take(bytes) -> offset
struct WsCursor {
    size_t off = 0;
    size_t operator()(size_t bytes) { const size_t o = off; off += align_up(bytes, 256); return o; }
};

// What every tower's kernels ask of (width, heads): 64-wide heads (the attention kernels), a width that is a multiple of
// 128 up to 1024 (LayerNorm, the GEMM tiles).  Each caller words its own error.
enum { SHAPE_OK = 0, SHAPE_HEAD_DIM, SHAPE_WIDTH };
static inline int check_width_heads(int width, int heads) {
    if (heads <= 0 || width != heads * 64) return SHAPE_HEAD_DIM;
    return (width % 128 != 0 || width > 1024) ? SHAPE_WIDTH : SHAPE_OK;
}

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

// the workspace of mpreid_vit_forward (byte offsets; every region 256-byte aligned)
struct VitLayout {
    int L, P, M, Mpad, MPpad, Kp, Bpad;
    size_t patches, x, a, qkv, hbuf, x_cls, a_cls, h_cls, y_cls, total;
};
VitLayout vit_layout(const mpreid_vit_cfg *c, int B);
int vit_check_cfg(const mpreid_vit_cfg *c);   // MPREID_ERR_ARG / MPREID_ERR_UNSUPPORTED with the error text set

// The image tower's embedded sequence in the split precision, what the forward launches in front of ln_pre: the patch
// gather into `patches` (fp16 pairs [MPpad][hi(Kp) | lo(Kp)]), conv1 + positional embedding, the CLS row (+ cv_emb).
// x [Mpad][W] fp32 = ln_pre's input.  `in` has passed mpreid_check_image_in.
int vit_embed_tokens(const mpreid_vit_cfg *cfg, const mpreid_vit_weights *w, const mpreid_image_in &in, int B, const float *cv_emb,
                     const VitLayout &v, _Float16 *patches, float *x, hipStream_t stream);
// out = LayerNorm(x) in fp32 over `rows` rows of W (layernorm_kernel<0>; out may be x)
int vit_layernorm_f32(const float *x, int64_t rows, int W, const float *g, const float *b, float *out, hipStream_t stream);

// One unmasked split-precision residual block over all M rows of x, in place (what mpreid_vit_forward runs per layer in
// front of the tail), and its two halves for the backward sweep, as text_block / text_block_recompute are for the causal
// tower.  vit_block_attention: qkv = q | k | v of ln_1(x) in fp32, a = the attention output as fp16 pairs [hi(W) | lo(W)];
// x is not written.  vit_block_mlp_recompute: x += out_proj(a) (the block's mid-point), a = ln_2(x) as pairs,
// u [Mpad][4W] = the FC1 pre-activation in fp32; FC2 is not run.
int vit_block(const mpreid_vit_cfg *cfg, int B, const mpreid_vit_layer &ly, float *x, _Float16 *a, float *qkv, _Float16 *hbuf,
              int M, int Mpad, hipStream_t stream);
int vit_block_attention(const mpreid_vit_cfg *cfg, int B, const mpreid_vit_layer &ly, const float *x, _Float16 *a, float *qkv,
                        int M, int Mpad, hipStream_t stream);
int vit_block_mlp_recompute(const mpreid_vit_cfg *cfg, int B, const mpreid_vit_layer &ly, float *x, _Float16 *a, float *u, int M,
                            int Mpad, hipStream_t stream);
// vit_block_mid: only x += out_proj(a), a = ln_2(x) as pairs (what an MoE block runs in front of its router and experts)
int vit_block_mid(const mpreid_vit_cfg *cfg, int B, const mpreid_vit_layer &ly, float *x, _Float16 *a, int M, int Mpad,
                  hipStream_t stream);
// the checks of an MoE tower call (vit.hip): the tower's shape, the row limit at this batch, the gate, every MoE block
int vit_check_moe_call(const mpreid_vit_cfg *cfg, const mpreid_vit_moe *moe, int B);

// text_grad.hip: the kernels the image tower's sweep borrows
int launch_layernorm_backward(const float *x, const float *dy, const float *g, int64_t rows, int W, bool acc, float *out,
                              hipStream_t s);
int launch_quickgelu_backward(const float *u, float *d, int64_t n4, hipStream_t s);

// The head of every tower (vit.hip): LayerNorm of ONE row per item, then that row @ proj.
//   x        fp32, item b at x + b * row_stride; its row is row 0 (row_of == nullptr: the CLS row) or row_of[b], device data
//            clamped into [0, L-1] (the text tower's end-of-text row).  Rows are W wide.
//   y        [B][W] fp32 scratch: the normalised rows
//   out      row stride out_stride; the projection lands at column out_col.  ln_to_out: the normalised row is also written
//            to out[b][0:W] (the image towers' concat [ln_post(CLS) | CLS @ proj]; out_stride = W + out_dim, out_col = W)
//   bn_* / bnp_*  optional eval-BatchNorm necks on the two halves (nullptr: none)
int tower_head(const float *x, int64_t row_stride, const int32_t *row_of, int L, int B, int W, int out_dim, const float *ln_g,
               const float *ln_b, const float *proj, const float *bn_s, const float *bn_b, const float *bnp_s,
               const float *bnp_b, float *y, float *out, int out_stride, int out_col, bool ln_to_out, hipStream_t stream);

// distance.hip: C[M][N] (row stride ldc) = A[M][K] x W[N][K]^T (+ bias[N]); exact fp32, k ascending, any M, N, K
int mpreid_gemm_f32_linear(const float *A, const float *Wt, int64_t M, int64_t N, int K, const float *bias, float *C,
                           int64_t ldc, int epi, hipStream_t stream);
enum { F32_LIN = 2, F32_LIN_GELU = 3, F32_LIN_RES = 4 };   // distance.hip: EPI_LIN*
