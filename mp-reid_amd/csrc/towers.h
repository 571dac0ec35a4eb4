// towers.h — what the tower files share: csrc/vit.hip (the image towers, the residual-block driver, the head), csrc/text.hip
// (the text tower's forward), csrc/text_grad.hip (mpreid_text_backward) and csrc/vit_grad.hip (mpreid_vit_backward and the
// differentiation of a block).  The block driver (block_attention_part / block_mlp_part) stays in vit.hip and is entered
// through the tower_block* functions below; a block is differentiated in ONE place, block_mlp_backward /
// block_attention_backward of vit_grad.hip, which both sweeps call, so each differentiates the activations its forward
// really produces.
#pragma once
#include "common.h"

// What every tower's kernels ask of (width, heads): 64-wide heads (the attention kernels), a width that is a multiple of
// 128 up to 1024 (LayerNorm, the GEMM tiles).  Each caller words its own error.
enum { SHAPE_OK = 0, SHAPE_HEAD_DIM, SHAPE_WIDTH };
static inline bool row_width_ok(int width) { return width >= 128 && width % 128 == 0 && width <= 1024; }
static inline int check_width_heads(int width, int heads) {
    if (heads <= 0 || width != heads * 64) return SHAPE_HEAD_DIM;
    return row_width_ok(width) ? SHAPE_OK : SHAPE_WIDTH;
}
// the width rule alone, for the row kernels' own entry points: MPREID_ERR_UNSUPPORTED with the error text set
static inline int check_row_width(const char *who, int width) {
    if (row_width_ok(width)) return MPREID_OK;
    mpreid_set_error("%s: width %d is not a multiple of 128 in 128..1024", who, width);
    return MPREID_ERR_UNSUPPORTED;
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
                     const VitLayout &v, _Float16 *patches, float *x, bool split, hipStream_t stream);
// out = LayerNorm(x) in fp32 over `rows` rows of W (layernorm_kernel<0>; out may be x)
int vit_layernorm_f32(const float *x, int64_t rows, int W, const float *g, const float *b, float *out, hipStream_t stream);

// The shape of a tower's residual blocks: what the block driver and the differentiation of a block need to know of a tower
struct BlockShape {
    int W, heads, B, L;   // width, heads, batch, tokens per item
    bool causal;          // the text tower's mask; false: the image towers' unmasked attention
    int M() const { return B * L; }
};
// One split-precision residual block over the M rows of x, in place (what mpreid_text_forward and mpreid_vit_forward run per
// layer, the latter in front of its tail), and its parts for the backward sweeps and the MoE blocks.  Mpad: the GEMMs' row
// count.  a: fp16 pairs [Mpad][2W]; qkv: fp32 [Mpad][3W]; hbuf: fp16 pairs [Mpad][8W].
// tower_block_attention: qkv = q | k | v of ln_1(x) in fp32, a = the attention output as fp16 pairs [hi(W) | lo(W)]; x is not
// written.  tower_block_mid: x += out_proj(a) (the block's mid-point), a = ln_2(x) as pairs (what an MoE block runs in front
// of its router and experts).  tower_block_mlp_recompute: tower_block_mid, then u [Mpad][4W] = the FC1 pre-activation in fp32
// (FC1 with GE_S_BIAS_F32 in place of GE_S_BIAS_GELU); FC2 is not run.
int tower_block(const BlockShape &s, const mpreid_vit_layer &ly, float *x, _Float16 *a, float *qkv, _Float16 *hbuf, int Mpad,
                hipStream_t stream);
int tower_block_attention(const BlockShape &s, const mpreid_vit_layer &ly, const float *x, _Float16 *a, float *qkv, int Mpad,
                          hipStream_t stream);
int tower_block_mid(const BlockShape &s, const mpreid_vit_layer &ly, float *x, _Float16 *a, int Mpad, hipStream_t stream);
int tower_block_mlp_recompute(const BlockShape &s, const mpreid_vit_layer &ly, float *x, _Float16 *a, float *u, int Mpad,
                              hipStream_t stream);
// the checks of an MoE tower call (vit.hip): the tower's shape, the row limit at this batch, the gate, every MoE block
int vit_check_moe_call(const mpreid_vit_cfg *cfg, const mpreid_vit_moe *moe, int B);

// text_grad.hip: the fp32 gradient kernels both sweeps launch; the attention gradient is the causal tower's (Q, K, V and dO
// of a head resident in LDS), d_qkv [B * L][3W] = dq | dk | dv
int launch_layernorm_backward(const float *x, const float *dy, const float *g, int64_t rows, int W, bool acc, float *out,
                              hipStream_t s);
int launch_quickgelu_backward(const float *u, float *d, int64_t n4, hipStream_t s);
int launch_causal_attention_backward(const float *qkv, const float *d_o, int B, int L, int W, int heads, float *d_qkv,
                                     hipStream_t s);

// What every backward sweep keeps behind its forward's regions, in this order; row: the bytes of one fp32 [Mpad][W] buffer
struct SweepRegions { size_t xs, dx, dh, t, dqkv; };
static inline SweepRegions take_sweep_regions(WsCursor &take, size_t row, int layers) {
    SweepRegions r;
    r.xs = take(row * (size_t)layers);   // x_l, the input of block l, l = 0 .. layers - 1
    r.dx = take(row);                    // the gradient of the residual stream
    r.dh = take(4 * row);                // the gradient of the MLP's hidden layer
    r.t = take(row);                     // the gradient of a LayerNorm output / of the attention output; ln_1(x_l)
    r.dqkv = take(3 * row);
    return r;
}

// The differentiation of one residual block (vit_grad.hip), in the two halves of the forward driver.  The state of a call:
// x holds x_l on entry to the sweep's recompute and the block's mid-point from block_mlp_backward on; a, qkv, u as
// tower_block_attention / tower_block_mlp_recompute leave them; dx the gradient of the residual stream, updated in place.
// Only a weight gradient reads aot (the attention output transposed, written by the sweep), at / bt (dY^T, X^T: [cols][Mp4],
// Mp4 = M rounded up to 4), and only a column sum reads red; the unmasked attention gradient needs stats.  A sweep without
// parameter gradients (an all-NULL mpreid_vit_layer_grads; the text tower's) leaves those four NULL: nothing is launched and
// no buffer touched for a gradient that is not asked for.
struct BlockGrad {
    BlockShape s;
    int Mpad;
    int64_t Mp4;
    hipStream_t stream;
    _Float16 *a;
    float *x, *qkv, *u, *dx, *dh, *t, *dqkv, *aot, *at, *bt;
    void *stats, *red;
};
// x_{l+1} = x_mid + c_proj(quickgelu(c_fc(ln_2(x_mid)))): recomputes x_mid, ln_2 and u; dx = d/dx_{l+1} -> t = the gradient
// of ln_2's output; writes g.proj_w, g.proj_b, g.fc_w, g.fc_b where asked
int block_mlp_backward(const BlockGrad &c, const mpreid_vit_layer &ly, const mpreid_text_layer_t &lt,
                       const mpreid_vit_layer_grads &g);
// ln_2 (t as the MLP half, dense or MoE, left it), then x_mid = x_l + out_proj(attention(in_proj(ln_1(x_l)))): dx = d/dx_l on
// return; the attention gradient is the causal or the unmasked kernel by c.s.causal; writes the other eight members of g
int block_attention_backward(const BlockGrad &c, const mpreid_vit_layer &ly, const mpreid_text_layer_t &lt, const float *xl,
                             const mpreid_vit_layer_grads &g);

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
