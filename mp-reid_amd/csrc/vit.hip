// vit.hip — CLIP ViT-B/16 image encoder forward for gfx950: the patch gather, LayerNorm, the residual-block driver that the
// image, MoE and text towers share, the head of every tower (towers.h), and the fp16 / split / MoE / all-fp32 image forwards.
// The attention kernels are in attention.hip (attention.h), the text tower's forward in text.hip.
//
// Reference: model/clip/model.py:415-479 (VisionTransformer.forward), :278-281
// (ResidualAttentionBlock), :150-156 (LayerNorm, fp32 statistics), :159-161 (QuickGELU);
// model/make_model.py:81-115 (CLS of x12 and of x12 @ proj, eval BatchNorm necks, concat).
//
// Precision plan: residual stream, LayerNorm statistics, softmax and all accumulators fp32;
// GEMM operands (LN outputs, Q/K/V, attention output, MLP hidden, weights) fp16 -> MFMA.
//
// HBM layout (workspace, M = B*L tokens, padded to 128 rows):
//   patches fp16 [B*P pad][3*p*p]   im2col of the image, inner order (c, kh, kw)
//   x       fp32 [M pad][W]         residual stream
//   a       fp16 [M pad][W]         LN output, then attention output (GEMM A operands)
//   qkv     fp16 [M pad][3W]        in_proj output, q | k | v column blocks, head h = cols [64h, 64h+64)
//   hbuf    fp16 [M pad][4W]        MLP hidden after QuickGELU
// Kernels: im2col (HBM), GEMM+epilogues (MFMA, gemm_f16.hip), LayerNorm (HBM), attention (attention.hip: MFMA +
// LDS; L = 129 keys fit one workgroup; 256 < L <= MPREID_VIT_MAX_TOKENS streams K / V through LDS), head (L2).
#include <cstdlib>
#include <mutex>
#include <type_traits>

#include "attention.h"
#include "gemm_f16.h"
#include "image_in.h"
#include "moe.h"
#include "towers.h"

// ---------------------------------------------------------------------------------------------
// im2col: the image batch (image_in.h: fp32 or uint8, any view) -> patches [MPpad][3*p*p] fp16; rows >= B*P are zero.
// VIEW and the input type are template arguments: the view and ToTensor + Normalize are applied while gathering, in fp32,
// before the fp16 rounding, with no run-time branch in the throughput path.
// ---------------------------------------------------------------------------------------------
// SPLIT (the `split` precision mode): rows are fp16 pairs [hi(Kp) | lo(Kp)] with hi + lo = the fp32 value to ~2^-22
typedef _Float16 h8_t __attribute__((ext_vector_type(8)));
template <bool SPLIT>
__device__ __forceinline__ void store_patch_row(_Float16 *__restrict__ out, int64_t m, int Kp, int ch, const float (&v)[8]) {
    h8_t hi, lo;
    split_pairs<8>(v, hi, lo);
    if constexpr (SPLIT) {
        *reinterpret_cast<h8_t *>(out + m * 2 * Kp + ch * 8) = hi;
        *reinterpret_cast<h8_t *>(out + m * 2 * Kp + Kp + ch * 8) = lo;
    } else {
        *reinterpret_cast<h8_t *>(out + m * Kp + ch * 8) = hi;
    }
}

template <int VIEW, bool SPLIT, bool U8>
__global__ __launch_bounds__(256) void im2col_kernel(const mpreid_image_in in, int B, int H, int Wd, int p, int stride,
                                                     int h_res, int w_res, _Float16 *__restrict__ out, int mp_pad) {
    const int Kp = 3 * p * p;
    const int chunks = Kp / 8; // 8 consecutive kw per thread
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gid >= (int64_t)mp_pad * chunks) return;
    const int m = (int)(gid / chunks), ch = (int)(gid % chunks);
    const int P = h_res * w_res;
    float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (m < B * P) {
        const int b = m / P, pi = m % P;
        const int ph = pi / w_res, pw = pi % w_res;
        const int k = ch * 8;
        const int c = k / (p * p), kh = (k % (p * p)) / p, kw = k % p;
        const int y = ph * stride + kh, x0 = pw * stride + kw;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            o[j] = image_px_view<VIEW, U8 ? IMAGE_SRC_U8 : IMAGE_SRC_F32>(in, b, c, y, x0 + j, H, Wd);
    }
    store_patch_row<SPLIT>(out, m, Kp, ch, o);
}

// x[b*L + 0][:] = class_embedding + pos[0] (+ cv_emb[b])      model/clip/model.py:419-422
__global__ __launch_bounds__(256) void cls_token_kernel(const float *__restrict__ cls, const float *__restrict__ pos,
                                                        const float *__restrict__ cv, int B, int L, int W,
                                                        float *__restrict__ x) {
    const int b = blockIdx.x;
    for (int k = threadIdx.x; k < W; k += 256) {
        float v = cls[k];
        if (cv) v = v + cv[(int64_t)b * W + k];
        x[(int64_t)b * L * W + k] = v + pos[k];
    }
}

// ---------------------------------------------------------------------------------------------
// LayerNorm over the last dim (biased variance, eps 1e-5, fp32 stats); one wave per row.
// MODE 0: write fp32 (may alias the input: ln_pre is in place); 1: fp16 (GEMM operand); 2: fp16 pair [hi(W) | lo(W)]
// per row (GEMM operand of the `split` precision mode).
// ---------------------------------------------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(256) void layernorm_kernel(const float *__restrict__ x, int64_t rows, int W,
                                                        const float *__restrict__ gamma,
                                                        const float *__restrict__ beta, void *__restrict__ out,
                                                        int64_t row_stride_in) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float *xr = x + row * row_stride_in;
    float4 v[4]; // W <= 1024; statically unrolled so that v[] stays in registers
    bool act[4];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        act[i] = (i * 256 + lane * 4) < W;
        v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (act[i]) {
            typedef float ln_f4 __attribute__((ext_vector_type(4)));
            const ln_f4 t = __builtin_nontemporal_load(reinterpret_cast<const ln_f4 *>(xr + i * 256 + lane * 4));
            v[i] = make_float4(t[0], t[1], t[2], t[3]);
        }
        s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
    const float mean = s / (float)W;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (act[i]) {
            const float a = v[i].x - mean, b = v[i].y - mean, c = v[i].z - mean, d = v[i].w - mean;
            q += (a * a + b * b) + (c * c + d * d);
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) q += __shfl_xor(q, off, 64);
    const float rstd = 1.0f / __fsqrt_rn(q / (float)W + 1e-5f);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (!act[i]) continue;
        const int k = i * 256 + lane * 4;
        const float4 gm = *reinterpret_cast<const float4 *>(gamma + k);
        const float4 bt = *reinterpret_cast<const float4 *>(beta + k);
        float4 y;
        y.x = (v[i].x - mean) * rstd * gm.x + bt.x;
        y.y = (v[i].y - mean) * rstd * gm.y + bt.y;
        y.z = (v[i].z - mean) * rstd * gm.z + bt.z;
        y.w = (v[i].w - mean) * rstd * gm.w + bt.w;
        if (MODE == 1) {
            typedef _Float16 h4 __attribute__((ext_vector_type(4)));
            h4 o = {(_Float16)y.x, (_Float16)y.y, (_Float16)y.z, (_Float16)y.w};
            *reinterpret_cast<h4 *>(reinterpret_cast<_Float16 *>(out) + row * (int64_t)W + k) = o;
        } else if (MODE == 2) {
            typedef _Float16 h4 __attribute__((ext_vector_type(4)));
            h4 hi, lo;
            {
                const float yv[4] = {y.x, y.y, y.z, y.w};
                split_pairs<4>(yv, hi, lo);
            }
            _Float16 *orow = reinterpret_cast<_Float16 *>(out) + row * 2 * (int64_t)W;
            *reinterpret_cast<h4 *>(orow + k) = hi;
            *reinterpret_cast<h4 *>(orow + W + k) = lo;
        } else {
            *reinterpret_cast<float4 *>(reinterpret_cast<float *>(out) + row * (int64_t)W + k) = y;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// head of every tower (tower_head, towers.h): LayerNorm of one row per item, that row @ proj, optional eval-BN necks.
// Image towers: ln_post on the CLS row, concat -> [B][W + out_dim]  (model/clip/model.py:471-474, model/make_model.py:98-115)
// Text tower: ln_final on the end-of-text row, @ text_projection -> [B][out_dim]  (model/clip/model.py:617-619)
// ---------------------------------------------------------------------------------------------
constexpr int HEAD_IMGS = 2;   // (8 images per workgroup: 128 workgroups, 90 us at B = 508; 2: 508 workgroups)
// One wave per item: y[b][:] (fp32, for the projection) and, with out != nullptr, out[b][0:W] (through the neck, if any).
// The row is row 0 of item b (row_of == nullptr), or row row_of[b]: device data that is not validated (include/mpreid.h), so
// the index is clamped into [0, L-1] and the read stays inside x.  Rows are W wide.
__global__ __launch_bounds__(256) void head_ln_kernel(const float *__restrict__ x, int64_t row_stride,
                                                      const int32_t *__restrict__ row_of, int L, int B, int W,
                                                      const float *__restrict__ g, const float *__restrict__ bta,
                                                      const float *__restrict__ bn_s, const float *__restrict__ bn_b,
                                                      float *__restrict__ y, float *__restrict__ out, int out_stride) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const float *xr = x + (int64_t)b * row_stride;
    if (row_of) {
        int e = row_of[b];
        e = e < 0 ? 0 : (e > L - 1 ? L - 1 : e);
        xr += (int64_t)e * W;
    }
    float s = 0.f;
    for (int k = lane; k < W; k += 64) s += xr[k];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
    const float mean = s / (float)W;
    float q = 0.f;
    for (int k = lane; k < W; k += 64) {
        const float d = xr[k] - mean;
        q += d * d;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) q += __shfl_xor(q, off, 64);
    const float rstd = 1.0f / sqrtf(q / (float)W + 1e-5f);   // (sqrtf, not layernorm_kernel's __fsqrt_rn: part of the bits)
    for (int k = lane; k < W; k += 64) {
        const float v = (xr[k] - mean) * rstd * g[k] + bta[k];
        y[(int64_t)b * W + k] = v;
        if (out) out[(int64_t)b * out_stride + k] = bn_s ? fmaf(v, bn_s[k], bn_b[k]) : v;
    }
}

// out[b][out_col + o] = sum_k y[b][k] * proj[k][o]  (fp32, k ascending).  grid = (ceil(B / HEAD_IMGS), ceil(out_dim / 256));
// HEAD_IMGS rows of y sit in LDS, every thread owns one output column for those items.
__global__ __launch_bounds__(256) void head_proj_kernel(const float *__restrict__ y, int B, int W, int out_dim,
                                                        const float *__restrict__ proj, const float *__restrict__ bnp_s,
                                                        const float *__restrict__ bnp_b, float *__restrict__ out,
                                                        int out_stride, int out_col) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *ys = reinterpret_cast<float *>(smem); // [HEAD_IMGS][W]
    const int tid = threadIdx.x;
    const int b0 = blockIdx.x * HEAD_IMGS;
    for (int idx = tid; idx < HEAD_IMGS * W; idx += 256) {
        const int i = idx / W, k = idx - i * W;
        ys[idx] = (b0 + i < B) ? y[(int64_t)(b0 + i) * W + k] : 0.f;
    }
    __syncthreads();
    const int o = blockIdx.y * 256 + tid;
    if (o >= out_dim) return;
    float acc[HEAD_IMGS];
#pragma unroll
    for (int i = 0; i < HEAD_IMGS; ++i) acc[i] = 0.f;
#pragma unroll 8
    for (int k = 0; k < W; ++k) {
        const float pw = proj[(int64_t)k * out_dim + o];
#pragma unroll
        for (int i = 0; i < HEAD_IMGS; ++i) acc[i] = fmaf(ys[i * W + k], pw, acc[i]);
    }
#pragma unroll
    for (int i = 0; i < HEAD_IMGS; ++i) {
        const int b = b0 + i;
        if (b < B) out[(int64_t)b * out_stride + out_col + o] = bnp_s ? fmaf(acc[i], bnp_s[o], bnp_b[o]) : acc[i];
    }
}

int tower_head(const float *x, int64_t row_stride, const int32_t *row_of, int L, int B, int W, int out_dim, const float *ln_g,
               const float *ln_b, const float *proj, const float *bn_s, const float *bn_b, const float *bnp_s,
               const float *bnp_b, float *y, float *out, int out_stride, int out_col, bool ln_to_out, hipStream_t stream) {
    hipLaunchKernelGGL(head_ln_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, stream, x, row_stride, row_of, L, B, W, ln_g,
                       ln_b, bn_s, bn_b, y, ln_to_out ? out : nullptr, out_stride);
    hipLaunchKernelGGL(head_proj_kernel, dim3((unsigned)((B + HEAD_IMGS - 1) / HEAD_IMGS), (unsigned)((out_dim + 255) / 256)),
                       dim3(256), (size_t)HEAD_IMGS * W * 4, stream, y, B, W, out_dim, proj, bnp_s, bnp_b, out, out_stride, out_col);
    LAUNCH_CHECK();
    return MPREID_OK;
}

// the head of the image towers: ln_post on the CLS row (row 0 of every row_stride floats of x), concat with CLS @ proj
static int image_head(const mpreid_vit_cfg *cfg, const mpreid_vit_weights *w, const float *x, int64_t row_stride, int B, float *y,
                      float *out, hipStream_t stream) {
    const bool neck = cfg->neck_after != 0 && w->bn_scale && w->bn_proj_scale;
    const int W = cfg->width;
    return tower_head(x, row_stride, nullptr, 1, B, W, cfg->out_dim, w->ln_post_g, w->ln_post_b, w->proj,
                      neck ? w->bn_scale : nullptr, neck ? w->bn_shift : nullptr, neck ? w->bn_proj_scale : nullptr,
                      neck ? w->bn_proj_shift : nullptr, y, out, W + cfg->out_dim, W, true, stream);
}

// CLS rows of the residual stream / attention output -> compact [Bpad][W] buffers (last block only)
// (aw = row length of a in halfs: W, or 2W for the fp16 pairs of the split mode)
__global__ __launch_bounds__(256) void gather_cls_kernel(const float *__restrict__ x, const _Float16 *__restrict__ a,
                                                         int B, int L, int W, int aw, float *__restrict__ x_cls,
                                                         _Float16 *__restrict__ a_cls) {
    const int b = blockIdx.x;
    for (int k = threadIdx.x; k < W; k += 256) x_cls[(int64_t)b * W + k] = x[(int64_t)b * L * W + k];
    for (int k = threadIdx.x; k < aw; k += 256) a_cls[(int64_t)b * aw + k] = a[(int64_t)b * L * aw + k];
}

// ---------------------------------------------------------------------------------------------
// host driver
// ---------------------------------------------------------------------------------------------
VitLayout vit_layout(const mpreid_vit_cfg *c, int B) {
    VitLayout v{};
    v.P = c->h_res * c->w_res;
    v.L = v.P + 1;
    v.M = B * v.L;
    v.Mpad = (int)align_up((size_t)v.M, 256);   // 256-row tiles of the big GEMM kernel
    v.MPpad = (int)align_up((size_t)B * v.P, 256);
    v.Kp = 3 * c->patch * c->patch;
    WsCursor take;
    const size_t W = (size_t)c->width;
    // split precision mode: every GEMM operand is an fp16 pair (2x the halfs per row), q | k | v are fp32
    const size_t pr = c->precision != MPREID_VIT_F16 ? 2 : 1;
    v.patches = take((size_t)v.MPpad * v.Kp * 2 * pr);
    v.x = take((size_t)v.Mpad * W * 4);
    v.a = take((size_t)v.Mpad * W * 2 * pr);
    v.qkv = take((size_t)v.Mpad * 3 * W * 2 * pr);
    v.hbuf = take((size_t)v.Mpad * 4 * W * 2 * pr);
    v.Bpad = (int)align_up((size_t)B, GBM);
    v.x_cls = take((size_t)v.Bpad * W * 4);
    v.a_cls = take((size_t)v.Bpad * W * 2 * pr);
    v.h_cls = take((size_t)v.Bpad * 4 * W * 2 * pr);
    v.y_cls = take((size_t)v.Bpad * W * 4);
    v.total = take.off;
    return v;
}

int vit_check_cfg(const mpreid_vit_cfg *c) {
    ARG_CHECK(c != nullptr);
    ARG_CHECK(c->width > 0 && c->heads > 0 && c->layers >= 0 && c->out_dim > 0);
    if (c->precision == 2) {   // MPREID_VIT_SPLIT_LNFOLD of rounds 3: see include/mpreid.h
        mpreid_set_error("the folded-LayerNorm form of the split mode was removed in round 4 (not faster than MPREID_VIT_SPLIT, and not "
                         "reproducible run to run at small batches); use MPREID_VIT_SPLIT");
        return MPREID_ERR_UNSUPPORTED;
    }
    ARG_CHECK(c->precision == MPREID_VIT_F16 || c->precision == MPREID_VIT_SPLIT);
    const int shape = check_width_heads(c->width, c->heads);
    if (shape == SHAPE_HEAD_DIM) {
        mpreid_set_error("head dim must be 64 (width %d, heads %d)", c->width, c->heads);
        return MPREID_ERR_UNSUPPORTED;
    }
    if (shape != SHAPE_OK || (3 * c->patch * c->patch) % 64 != 0 || c->patch % 8 != 0) {
        mpreid_set_error("unsupported ViT geometry (width %d, patch %d)", c->width, c->patch);
        return MPREID_ERR_UNSUPPORTED;
    }
    ARG_CHECK(c->h_res == (c->img_h - c->patch) / c->stride + 1 && c->w_res == (c->img_w - c->patch) / c->stride + 1);
    if (c->h_res * c->w_res + 1 > MPREID_VIT_MAX_TOKENS) {
        mpreid_set_error("token count %d > %d (MPREID_VIT_MAX_TOKENS, 512 x 512 at stride 16) not supported by the attention kernels",
                         c->h_res * c->w_res + 1, MPREID_VIT_MAX_TOKENS);
        return MPREID_ERR_UNSUPPORTED;
    }
    return MPREID_OK;
}

extern "C" size_t mpreid_vit_workspace_bytes(const mpreid_vit_cfg *cfg, int batch) {
    if (!cfg || batch <= 0) return 0;
    return vit_layout(cfg, batch).total;
}

// The MoE forward's share of the workspace, behind the dense layout: the routing of block 0 and the routed-MLP workspace
struct VitMoeLayout {
    MoeLayout m;
    size_t sel, w, moe, logits, route, total;   // logits / route: the training forward's router logits and l_aux tables
    float *logits_dst = nullptr;                // where block 0's router writes its logits (nullptr: nowhere)
};
static VitMoeLayout vit_moe_layout(const mpreid_vit_cfg *c, const mpreid_vit_moe *moe, int B, bool train = false) {
    const VitLayout v = vit_layout(c, B);
    VitMoeLayout o{};
    o.m = moe_layout((int64_t)v.M, c->width, moe->num_experts, moe->top_k);
    WsCursor take{v.total};
    o.sel = take((size_t)v.M * moe->top_k * 4);
    o.w = take((size_t)v.M * moe->top_k * 4);
    o.moe = take(o.m.total);   // (a multiple of 256 already: moe_layout)
    if (train) {               // mpreid_vit_forward_train_moe: the router's logits and the tables of l_aux
        o.logits = take((size_t)v.M * moe->num_experts * 4);
        o.route = take(moe_route_grad_bytes((int64_t)v.M, moe->num_experts));
    }
    o.total = take.off;
    return o;
}

// The residual block of the fp16 / split towers, x += out_proj(attn(ln_1(x))); x += mlp(ln_2(x)): the ONE launch sequence of
// the image tower (dense and MoE) and the text tower.  Two parts: the image tower's CLS-only tail block gathers the CLS rows
// between them and runs the second part on those alone.
struct BlockCtx {
    hipStream_t stream;
    bool split;   // every linear layer runs hi.hi' + lo.hi' + hi.lo' over fp16 pairs (gemm_f16.h GE_S_*); q | k | v are fp32
    int pr;       // halfs per logical element of a GEMM operand row: 2 in the split mode, else 1
    int W, heads, B, L;
};
enum AttnKind { ATTN_ALL_ROWS, ATTN_CLS_TILE, ATTN_CAUSAL };   // which query rows / which mask the block's attention runs

static int linear(const BlockCtx &c, GemmArgs &g, int kdim, float wscale, int epi_f16, int epi_split) {
    g.K = c.pr * kdim;
    if (c.split) {
        g.kseg = kdim;
        g.oscale = wscale;
    }
    return launch_gemm_f16(g, c.split ? epi_split : epi_f16, c.stream);
}

// a = ln(x) as the next GEMM's operand (fp16, or the fp16 pair of the split mode)
static void block_layernorm(const BlockCtx &c, const float *x, int rows, const float *g, const float *b, _Float16 *a) {
    const dim3 grid((unsigned)((rows + 3) / 4));
    if (c.split)
        hipLaunchKernelGGL(layernorm_kernel<2>, grid, dim3(256), 0, c.stream, x, (int64_t)rows, c.W, g, b, (void *)a, (int64_t)c.W);
    else
        hipLaunchKernelGGL(layernorm_kernel<1>, grid, dim3(256), 0, c.stream, x, (int64_t)rows, c.W, g, b, (void *)a, (int64_t)c.W);
}

// the attention of a block inside its profiling bracket: class (MPREID_PROF_ATTENTION, M, CLS tile only, pr)
static int attention_profiled(const BlockCtx &c, const void *qkv, _Float16 *out, AttnKind kind) {
    const int64_t M = (int64_t)c.B * c.L;
    const int cls = kind == ATTN_CLS_TILE ? 1 : 0;   // q_tiles of the dispatchers: the first 16-query tile, or 0 = all rows
    void *ptok = mpreid_prof_begin(c.stream);
    int rc;
    if (kind == ATTN_CAUSAL)
        rc = attention_causal_dispatch(reinterpret_cast<const float *>(qkv), c.B, c.L, c.W, c.heads, out, c.stream);
    else if (c.split)
        rc = attention_split_dispatch(reinterpret_cast<const float *>(qkv), c.B, c.L, c.W, c.heads, out, cls, c.stream);
    else
        rc = attention_dispatch(reinterpret_cast<const _Float16 *>(qkv), c.B, c.L, c.W, c.heads, out, cls, c.stream);
    mpreid_prof_end(ptok, c.stream, MPREID_PROF_ATTENTION, M, cls, c.pr, attention_bytes(M, cls ? (int64_t)c.B * 16 : M, c.W, c.pr));
    return rc;
}

// a = attn(in_proj(ln_1(x))) over the M rows of x (Mpad: the GEMM's row count)
static int block_attention_part(const BlockCtx &c, const mpreid_vit_layer &ly, const float *x, _Float16 *a, void *qkv, int M,
                                int Mpad, AttnKind kind) {
    const int W = c.W;
    void *ptok = mpreid_prof_begin(c.stream);
    block_layernorm(c, x, M, ly.ln1_g, ly.ln1_b, a);
    mpreid_prof_end(ptok, c.stream, MPREID_PROF_LAYERNORM, M, W, c.pr, (double)M * W * (4.0 + 2.0 * c.pr));
    LAUNCH_CHECK();
    GemmArgs g{};
    g.A = a; g.W = (const _Float16 *)ly.in_proj_w; g.M = Mpad; g.N = 3 * W;
    g.out = qkv; g.ldo = 3 * W; g.bias = ly.in_proj_b;
    const int rc = linear(c, g, W, ly.in_proj_s, GE_BIAS_F16, GE_S_BIAS_F32);
    return rc ? rc : attention_profiled(c, qkv, a, kind);
}

// xr += out_proj(ar) (the block's mid-point); ar = ln_2(xr) as the MLP's operand
static int block_mid_part(const BlockCtx &c, const mpreid_vit_layer &ly, float *xr, _Float16 *ar, int rows, int rows_pad) {
    const int W = c.W;
    GemmArgs g{};
    g.A = ar; g.W = (const _Float16 *)ly.out_proj_w; g.M = rows_pad; g.N = W;
    g.out = xr; g.ldo = W; g.bias = ly.out_proj_b;
    const int rc = linear(c, g, W, ly.out_proj_s, GE_BIAS_RES, GE_S_BIAS_RES);
    if (rc) return rc;
    block_layernorm(c, xr, rows, ly.ln2_g, ly.ln2_b, ar);
    LAUNCH_CHECK();
    return MPREID_OK;
}

// xr += out_proj(ar); xr += mlp(ln_2(xr)) over `rows` rows (rows_pad: the GEMMs' row count; hr: the MLP's hidden buffer).
// Blocks l < moe->moe_layers of an MoE tower (moe != nullptr; vm places its workspace share behind base) run router and
// dispatch (l == 0 only), grouped FC1 / FC2 and combine (csrc/moe.hip) in place of FC1 and FC2
// fc1_f32 (the backward sweeps, tower_block_mlp_recompute): FC1 leaves its pre-activation there in fp32 [rows_pad][4W]
// and the part ends before FC2, with xr = the block's mid-point
static int block_mlp_part(const BlockCtx &c, const mpreid_vit_layer &ly, float *xr, _Float16 *ar, _Float16 *hr, int rows,
                          int rows_pad, const mpreid_vit_moe *moe, int l, const VitMoeLayout *vm, char *base,
                          float *fc1_f32 = nullptr) {
    const int W = c.W;
    int rc;
    if ((rc = block_mid_part(c, ly, xr, ar, rows, rows_pad))) return rc;
    GemmArgs g{};
    if (moe && l < moe->moe_layers) {
        char *mws = base + vm->moe;
        int32_t *sel = (int32_t *)(base + vm->sel);
        float *rw = (float *)(base + vm->w);
        if (l == 0) {
            if ((rc = moe_route_launch(xr, (int64_t)rows, W, ly.ln2_g, ly.ln2_b, moe->layers[0].gate_w, moe->num_experts,
                                       moe->top_k, sel, rw, vm->logits_dst, c.stream)))
                return rc;
            if ((rc = moe_dispatch_launch(sel, rw, vm->m, mws, c.stream))) return rc;
        }
        return moe_mlp_launch(ar, vm->m, &moe->layers[l], xr, mws, c.stream);
    }
    g = GemmArgs{};
    g.A = ar; g.W = (const _Float16 *)ly.fc_w; g.M = rows_pad; g.N = 4 * W;
    g.bias = ly.fc_b;
    if (fc1_f32) {
        ARG_CHECK(c.split);   // there is no fp32 epilogue among the fp16 mode's
        g.out = fc1_f32; g.ldo = 4 * W;
        return linear(c, g, W, ly.fc_s, GE_BIAS_F16, GE_S_BIAS_F32);
    }
    g.out = hr; g.ldo = c.pr * 4 * W;
    if ((rc = linear(c, g, W, ly.fc_s, GE_BIAS_GELU, GE_S_BIAS_GELU))) return rc;
    g = GemmArgs{};
    g.A = hr; g.W = (const _Float16 *)ly.proj_w; g.M = rows_pad; g.N = W;
    g.out = xr; g.ldo = W; g.bias = ly.proj_b;
    return linear(c, g, 4 * W, ly.proj_s, GE_BIAS_RES, GE_S_BIAS_RES);
}

// The embedded sequence, ln_pre's input: patch gather, conv1 (no bias) + positional embedding, the CLS row (+ cv_emb)
int vit_embed_tokens(const mpreid_vit_cfg *cfg, const mpreid_vit_weights *w, const mpreid_image_in &in, int B, const float *cv_emb,
                     const VitLayout &v, _Float16 *patches, float *x, bool split, hipStream_t stream) {
    const int W = cfg->width, L = v.L;
    const int64_t threads = (int64_t)v.MPpad * (v.Kp / 8);
    const dim3 grid((unsigned)((threads + 255) / 256));
#define MPREID_IM2COL(V, S, U)                                                                                         \
    case (V) * 4 + (S) * 2 + (U):                                                                                      \
        hipLaunchKernelGGL((im2col_kernel<V, S, U>), grid, dim3(256), 0, stream, in, B, cfg->img_h, cfg->img_w,        \
                           cfg->patch, cfg->stride, cfg->h_res, cfg->w_res, patches, v.MPpad);                         \
        break;
#define MPREID_IM2COL_V(V)                                                                                             \
    MPREID_IM2COL(V, false, false) MPREID_IM2COL(V, false, true) MPREID_IM2COL(V, true, false) MPREID_IM2COL(V, true, true)
    switch (in.view * 4 + (split ? 2 : 0) + (in.u8_hwc_dev ? 1 : 0)) {   // (in.view is 0..3: mpreid_check_image_in)
        MPREID_IM2COL_V(0) MPREID_IM2COL_V(1) MPREID_IM2COL_V(2) MPREID_IM2COL_V(3)
    }
#undef MPREID_IM2COL_V
#undef MPREID_IM2COL
    LAUNCH_CHECK();
    GemmArgs g{};
    g.A = patches;
    g.W = (const _Float16 *)w->conv_w;
    g.M = v.MPpad;
    g.N = W;
    g.out = x;
    g.ldo = W;
    g.aux = w->pos_emb;
    g.m_valid = B * v.P;
    g.P = v.P;
    g.L = L;
    const int rc = linear(BlockCtx{stream, split, split ? 2 : 1, W, cfg->heads, B, L}, g, v.Kp, w->conv_s, GE_PATCH, GE_S_PATCH);
    if (rc) return rc;
    hipLaunchKernelGGL(cls_token_kernel, dim3((unsigned)B), dim3(256), 0, stream, w->class_emb, w->pos_emb, cv_emb, B, L, W, x);
    LAUNCH_CHECK();
    return MPREID_OK;
}

// The three features of the training forward (mpreid_vit_forward_train) in place of `out`: no neck, f | f_proj apart
struct TrainOut {
    float *f_last, *f, *f_proj;   // [B][W], [B][W], [B][out_dim]
    float *logits, *l_aux;        // an MoE tower's router logits [B * L][E] and load-balancing loss [1]; either may be nullptr
};

// moe == nullptr: the dense tower (mpreid_vit_forward).  Otherwise blocks l < moe->moe_layers run the routed MLP.
// tr != nullptr: the training forward -- the same launches, plus one copy of the B CLS rows in front of the last block.
static int vit_forward_impl(const mpreid_vit_cfg *cfg, const mpreid_vit_weights *w, const mpreid_vit_moe *moe,
                            const mpreid_image_in *img, int B, const float *cv_emb, float *out, void *ws, size_t ws_bytes,
                            mpreid_stream_t stream_, const TrainOut *tr = nullptr) {
    int rc = vit_check_cfg(cfg);
    if (rc) return rc;
    if (tr && (cfg->precision != MPREID_VIT_SPLIT || cfg->layers < 1)) {
        mpreid_set_error("the training forward runs the dense tower in the split precision with at least one layer "
                         "(precision %d, layers %d)", cfg->precision, cfg->layers);
        return MPREID_ERR_UNSUPPORTED;
    }
    mpreid_image_in in;
    if ((rc = mpreid_check_image_in(img, &in))) return rc;
    ARG_CHECK(w && (out || tr) && B > 0 && w->layers);
    const VitLayout v = vit_layout(cfg, B);
    const int n_moe = moe ? moe->moe_layers : 0;
    VitMoeLayout vm{};
    if (moe) {
        ARG_CHECK(((uintptr_t)ws & 255) == 0 && ((uintptr_t)out & 3) == 0 && ((uintptr_t)cv_emb & 3) == 0);
        vm = vit_moe_layout(cfg, moe, B, tr != nullptr);
    }
    const size_t ws_need = moe ? vm.total : v.total;
    if (!ws || ws_bytes < ws_need) {
        mpreid_set_error("vit workspace too small: %zu < %zu", ws_bytes, ws_need);
        return MPREID_ERR_WORKSPACE;
    }
    hipStream_t stream = (hipStream_t)stream_;
    const int W = cfg->width, L = v.L;
    char *base = (char *)ws;
    _Float16 *patches = (_Float16 *)(base + v.patches);
    float *x = (float *)(base + v.x);
    _Float16 *a = (_Float16 *)(base + v.a);
    _Float16 *qkv = (_Float16 *)(base + v.qkv);
    _Float16 *hbuf = (_Float16 *)(base + v.hbuf);
    float *x_cls = (float *)(base + v.x_cls);
    _Float16 *a_cls = (_Float16 *)(base + v.a_cls);
    _Float16 *h_cls = (_Float16 *)(base + v.h_cls);
    float *y_cls = (float *)(base + v.y_cls);
    // (an MoE block in the last position runs on all rows: include/mpreid.h)
    const bool cls_last = cfg->cls_only_last != 0 && cfg->layers > 0 && n_moe < cfg->layers;
    const bool split = cfg->precision != MPREID_VIT_F16;
    const BlockCtx ctx{stream, split, split ? 2 : 1, W, cfg->heads, B, L};
    if (tr && moe && (tr->logits || tr->l_aux)) vm.logits_dst = (float *)(base + vm.logits);

    // patch embedding (conv1, no bias) + positional embedding; CLS row; ln_pre
    if ((rc = vit_embed_tokens(cfg, w, in, B, cv_emb, v, patches, x, split, stream))) return rc;
    hipLaunchKernelGGL(layernorm_kernel<0>, dim3((unsigned)((v.M + 3) / 4)), dim3(256), 0, stream, x, (int64_t)v.M, W,
                       w->ln_pre_g, w->ln_pre_b, (void *)x, (int64_t)W);
    LAUNCH_CHECK();
    for (int l = 0; l < cfg->layers; ++l) {
        const mpreid_vit_layer &ly = w->layers[l];
        // in the last block only the CLS row reaches the output (model/make_model.py:98-100): the
        // attention runs the first query tile only and everything after it runs on the B CLS rows.
        const bool tail = cls_last && (l == cfg->layers - 1);
        if (tr && !moe && l == cfg->layers - 1)   // f_last: the CLS row of the last block's input (model/clip/model.py:458-468)
            HIP_TRY(hipMemcpy2DAsync(tr->f_last, (size_t)W * 4, x, (size_t)L * W * 4, (size_t)W * 4, (size_t)B,
                                     hipMemcpyDeviceToDevice, stream));
        if ((rc = block_attention_part(ctx, ly, x, a, qkv, v.M, v.Mpad, tail ? ATTN_CLS_TILE : ATTN_ALL_ROWS))) return rc;
        if (tail) {   // (never an MoE block)
            hipLaunchKernelGGL(gather_cls_kernel, dim3((unsigned)B), dim3(256), 0, stream, x, a, B, L, W, ctx.pr * W, x_cls, a_cls);
            LAUNCH_CHECK();
        }
        if ((rc = tail ? block_mlp_part(ctx, ly, x_cls, a_cls, h_cls, B, v.Bpad, moe, l, &vm, base)
                       : block_mlp_part(ctx, ly, x, a, hbuf, v.M, v.Mpad, moe, l, &vm, base)))
            return rc;
    }
    if (tr && moe) {
        // with MoE the tower hands out x11 = x12 = the transformer's output (model/clip/model.py:448-454): f_last is the CLS
        // row of the LAST block's OUTPUT
        const float *xo = cls_last ? x_cls : x;
        HIP_TRY(hipMemcpy2DAsync(tr->f_last, (size_t)W * 4, xo, cls_last ? (size_t)W * 4 : (size_t)L * W * 4, (size_t)W * 4,
                                 (size_t)B, hipMemcpyDeviceToDevice, stream));
        if (vm.logits_dst) {
            const size_t lbytes = (size_t)v.M * moe->num_experts * 4;
            if (tr->logits) HIP_TRY(hipMemcpyAsync(tr->logits, vm.logits_dst, lbytes, hipMemcpyDeviceToDevice, stream));
            if (tr->l_aux) {
                if ((rc = moe_route_backward_ws(vm.logits_dst, (const int32_t *)(base + vm.sel), (const float *)(base + vm.w),
                                                nullptr, v.M, moe->num_experts, moe->top_k, 0.f, nullptr, tr->l_aux,
                                                (const int *)(base + vm.moe + vm.m.meta) + MOE_META_COUNTS, base + vm.route,
                                                stream)))
                    return rc;
            }
        }
    }
    if (tr)   // the head's own kernels: the normalised rows land in f (the forward's scratch y), the projection in f_proj
        return tower_head(cls_last ? x_cls : x, cls_last ? (int64_t)W : (int64_t)L * W, nullptr, 1, B, W, cfg->out_dim,
                          w->ln_post_g, w->ln_post_b, w->proj, nullptr, nullptr, nullptr, nullptr, tr->f, tr->f_proj, cfg->out_dim,
                          0, false, stream);
    return image_head(cfg, w, cls_last ? x_cls : x, cls_last ? (int64_t)W : (int64_t)L * W, B, y_cls, out, stream);
}

extern "C" int mpreid_vit_forward_train(const mpreid_vit_cfg *cfg, const mpreid_vit_weights *w, const mpreid_image_in *img, int B,
                                        const float *cv_emb, float *f_last, float *f, float *f_proj, void *ws, size_t ws_bytes,
                                        mpreid_stream_t stream_) {
    ARG_CHECK(f_last && f && f_proj);
    ARG_CHECK((((uintptr_t)f_last | (uintptr_t)f | (uintptr_t)f_proj) & 3) == 0);
    const TrainOut tr{f_last, f, f_proj, nullptr, nullptr};
    return vit_forward_impl(cfg, w, nullptr, img, B, cv_emb, nullptr, ws, ws_bytes, stream_, &tr);
}

extern "C" int mpreid_vit_forward(const mpreid_vit_cfg *cfg, const mpreid_vit_weights *w, const mpreid_image_in *img, int B,
                                  const float *cv_emb, float *out, void *ws, size_t ws_bytes, mpreid_stream_t stream_) {
    return vit_forward_impl(cfg, w, nullptr, img, B, cv_emb, out, ws, ws_bytes, stream_);
}

// ---- MoE image encoder (include/mpreid.h; kernels in csrc/moe.hip) ----
static int vit_check_moe(const mpreid_vit_cfg *cfg, const mpreid_vit_moe *moe) {
    int rc = vit_check_cfg(cfg);
    if (rc) return rc;
    ARG_CHECK(moe != nullptr);
    if (cfg->precision != MPREID_VIT_SPLIT) {
        mpreid_set_error("the MoE image encoder runs in the split precision mode only (include/mpreid.h)");
        return MPREID_ERR_UNSUPPORTED;
    }
    if (moe->moe_layers < 0 || moe->moe_layers > cfg->layers) {
        mpreid_set_error("MoE: moe_layers %d outside 0 .. layers (%d)", moe->moe_layers, cfg->layers);
        return MPREID_ERR_UNSUPPORTED;
    }
    return moe_check_shape((int64_t)cfg->h_res * cfg->w_res + 1, cfg->width, moe->num_experts, moe->top_k);
}

extern "C" size_t mpreid_vit_workspace_bytes_moe(const mpreid_vit_cfg *cfg, const mpreid_vit_moe *moe, int batch) {
    if (!cfg || !moe || batch <= 0 || vit_check_moe(cfg, moe)) return 0;
    return vit_moe_layout(cfg, moe, batch).total;
}

// the checks of an MoE tower call that need the batch: the row limit, the gate, every MoE block's pointers
int vit_check_moe_call(const mpreid_vit_cfg *cfg, const mpreid_vit_moe *moe, int B) {
    int rc = vit_check_moe(cfg, moe);
    if (rc) return rc;
    ARG_CHECK(B > 0);
    if ((rc = moe_check_shape((int64_t)B * (cfg->h_res * cfg->w_res + 1), cfg->width, moe->num_experts, moe->top_k))) return rc;
    if (moe->moe_layers > 0) {
        ARG_CHECK(moe->layers != nullptr);
        ARG_CHECK(moe->layers[0].gate_w && ((uintptr_t)moe->layers[0].gate_w & 15) == 0);
        for (int l = 0; l < moe->moe_layers; ++l)
            if ((rc = moe_check_layer(&moe->layers[l]))) return rc;
    }
    return MPREID_OK;
}

extern "C" int mpreid_vit_forward_moe(const mpreid_vit_cfg *cfg, const mpreid_vit_weights *w, const mpreid_vit_moe *moe,
                                      const mpreid_image_in *img, int B, const float *cv_emb, float *out, void *ws,
                                      size_t ws_bytes, mpreid_stream_t stream_) {
    const int rc = vit_check_moe_call(cfg, moe, B);
    if (rc) return rc;
    return vit_forward_impl(cfg, w, moe, img, B, cv_emb, out, ws, ws_bytes, stream_);
}

static int vit_check_moe_train(const mpreid_vit_moe *moe) {
    if (moe->moe_layers < 1) {
        mpreid_set_error("the MoE training entry points need at least one MoE block (moe_layers %d): a tower without one is the "
                         "dense tower of mpreid_vit_forward_train / mpreid_vit_backward", moe->moe_layers);
        return MPREID_ERR_UNSUPPORTED;
    }
    return MPREID_OK;
}

extern "C" size_t mpreid_vit_forward_train_moe_workspace_bytes(const mpreid_vit_cfg *cfg, const mpreid_vit_moe *moe, int batch) {
    if (!cfg || !moe || batch <= 0 || vit_check_moe(cfg, moe) || vit_check_moe_train(moe)) return 0;
    return vit_moe_layout(cfg, moe, batch, true).total;
}

extern "C" int mpreid_vit_forward_train_moe(const mpreid_vit_cfg *cfg, const mpreid_vit_weights *w, const mpreid_vit_moe *moe,
                                            const mpreid_image_in *img, int B, const float *cv_emb, float *f_last, float *f,
                                            float *f_proj, float *logits_out, float *l_aux_out, void *ws, size_t ws_bytes,
                                            mpreid_stream_t stream_) {
    int rc = vit_check_moe_call(cfg, moe, B);
    if (rc) return rc;
    if ((rc = vit_check_moe_train(moe))) return rc;
    ARG_CHECK(f_last && f && f_proj);
    ARG_CHECK((((uintptr_t)f_last | (uintptr_t)f | (uintptr_t)f_proj | (uintptr_t)logits_out | (uintptr_t)l_aux_out) & 3) == 0);
    const TrainOut tr{f_last, f, f_proj, logits_out, l_aux_out};
    return vit_forward_impl(cfg, w, moe, img, B, cv_emb, nullptr, ws, ws_bytes, stream_, &tr);
}

// =============================================================================================
// All-fp32 encoder mode (SURVEY.md section 7 hard part 5: "expose an all-fp32 debug mode").
// The fp16-MFMA path above carries a relative feature error of ~4e-4 (operand rounding), which moves mAP by ~1e-4
// on hard data (tests/test_gpu_map_parity.py); this mode keeps every activation and weight in fp32 and runs the
// linear layers on the exact fp32 matrix instruction (gemm_f32_exact_kernel, k-ascending fmaf chains, ~100 TFLOP/s),
// the attention on fp32 vector FMAs.  ~4-5 k images/s: a parity / debugging mode, not the throughput path.
// Same structs as the fp16 entry points, but every *_w / conv_w pointer is an fp32 [out][in] matrix.
// =============================================================================================
// the image batch (image_in.h) -> patches [B*P][3*p*p] fp32, inner order (c, kh, kw); input type and view are run-time here:
// the all-fp32 mode is the parity / debugging mode, not a throughput path
__global__ __launch_bounds__(256) void im2col_f32_kernel(const mpreid_image_in in, int B, int H, int Wd, int p, int stride,
                                                         int h_res, int w_res, float *__restrict__ out) {
    const int Kp = 3 * p * p, P = h_res * w_res;
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gid >= (int64_t)B * P * Kp) return;
    const int m = (int)(gid / Kp), k = (int)(gid % Kp);
    const int b = m / P, pi = m % P, ph = pi / w_res, pw = pi % w_res;
    const int c = k / (p * p), kh = (k % (p * p)) / p, kw = k % p;
    out[gid] = image_px(in, in.view, b, c, ph * stride + kh, pw * stride + kw, H, Wd);
}

// x[b*L + 1 + p][:] = tok[b*P + p][:] + pos[1 + p][:]
__global__ __launch_bounds__(256) void patch_scatter_f32_kernel(const float *__restrict__ tok, const float *__restrict__ pos, int B,
                                                                int P, int L, int W, float *__restrict__ x) {
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gid >= (int64_t)B * P * W) return;
    const int m = (int)(gid / W), k = (int)(gid % W);
    const int b = m / P, pp = m % P;
    x[((int64_t)b * L + 1 + pp) * W + k] = tok[gid] + pos[(int64_t)(1 + pp) * W + k];
}

struct VitLayoutF32 {
    int L, P, M, Kp;
    size_t patches, x, a, qkv, hbuf, y_cls, total;
};
static VitLayoutF32 vit_layout_f32(const mpreid_vit_cfg *c, int B) {
    VitLayoutF32 v{};
    v.P = c->h_res * c->w_res;
    v.L = v.P + 1;
    v.M = B * v.L;
    v.Kp = 3 * c->patch * c->patch;
    WsCursor take;
    v.patches = take((size_t)B * v.P * v.Kp * 4);
    v.x = take((size_t)v.M * c->width * 4);
    v.a = take((size_t)v.M * c->width * 4);
    v.qkv = take((size_t)v.M * 3 * c->width * 4);
    v.hbuf = take((size_t)v.M * 4 * c->width * 4);
    v.y_cls = take((size_t)B * c->width * 4);
    v.total = take.off;
    return v;
}

extern "C" size_t mpreid_vit_workspace_bytes_f32(const mpreid_vit_cfg *cfg, int batch) {
    if (!cfg || batch <= 0) return 0;
    return vit_layout_f32(cfg, batch).total;
}

extern "C" int mpreid_vit_forward_f32(const mpreid_vit_cfg *cfg, const mpreid_vit_weights *w, const mpreid_image_in *img, int B,
                                      const float *cv_emb, float *out, void *ws, size_t ws_bytes, mpreid_stream_t stream_) {
    int rc = vit_check_cfg(cfg);
    if (rc) return rc;
    mpreid_image_in in;
    if ((rc = mpreid_check_image_in(img, &in))) return rc;
    ARG_CHECK(w && out && B > 0 && w->layers);
    const VitLayoutF32 v = vit_layout_f32(cfg, B);
    if (!ws || ws_bytes < v.total) {
        mpreid_set_error("vit fp32 workspace too small: %zu < %zu", ws_bytes, v.total);
        return MPREID_ERR_WORKSPACE;
    }
    hipStream_t stream = (hipStream_t)stream_;
    const int W = cfg->width, L = v.L;
    char *base = (char *)ws;
    float *patches = (float *)(base + v.patches), *x = (float *)(base + v.x), *a = (float *)(base + v.a);
    float *qkv = (float *)(base + v.qkv), *hbuf = (float *)(base + v.hbuf), *y_cls = (float *)(base + v.y_cls);
    {
        const int64_t n = (int64_t)B * v.P * v.Kp;
        hipLaunchKernelGGL(im2col_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, in, B, cfg->img_h,
                           cfg->img_w, cfg->patch, cfg->stride, cfg->h_res, cfg->w_res, patches);
        LAUNCH_CHECK();
        if ((rc = mpreid_gemm_f32_linear(patches, (const float *)w->conv_w, (int64_t)B * v.P, W, v.Kp, nullptr, a, W, F32_LIN,
                                         stream)))
            return rc;
        const int64_t n2 = (int64_t)B * v.P * W;
        hipLaunchKernelGGL(patch_scatter_f32_kernel, dim3((unsigned)((n2 + 255) / 256)), dim3(256), 0, stream, a, w->pos_emb, B,
                           v.P, L, W, x);
        hipLaunchKernelGGL(cls_token_kernel, dim3((unsigned)B), dim3(256), 0, stream, w->class_emb, w->pos_emb, cv_emb, B, L, W,
                           x);
        hipLaunchKernelGGL(layernorm_kernel<0>, dim3((unsigned)((v.M + 3) / 4)), dim3(256), 0, stream, x, (int64_t)v.M, W,
                           w->ln_pre_g, w->ln_pre_b, (void *)x, (int64_t)W);
        LAUNCH_CHECK();
    }
    for (int l = 0; l < cfg->layers; ++l) {
        const mpreid_vit_layer &ly = w->layers[l];
        hipLaunchKernelGGL(layernorm_kernel<0>, dim3((unsigned)((v.M + 3) / 4)), dim3(256), 0, stream, x, (int64_t)v.M, W,
                           ly.ln1_g, ly.ln1_b, (void *)a, (int64_t)W);
        LAUNCH_CHECK();
        if ((rc = mpreid_gemm_f32_linear(a, (const float *)ly.in_proj_w, v.M, 3 * W, W, ly.in_proj_b, qkv, 3 * W, F32_LIN, stream)))
            return rc;
        if ((rc = attention_f32_dispatch(qkv, B, L, W, cfg->heads, a, stream))) return rc;
        if ((rc = mpreid_gemm_f32_linear(a, (const float *)ly.out_proj_w, v.M, W, W, ly.out_proj_b, x, W, F32_LIN_RES, stream)))
            return rc;
        hipLaunchKernelGGL(layernorm_kernel<0>, dim3((unsigned)((v.M + 3) / 4)), dim3(256), 0, stream, x, (int64_t)v.M, W,
                           ly.ln2_g, ly.ln2_b, (void *)a, (int64_t)W);
        LAUNCH_CHECK();
        if ((rc = mpreid_gemm_f32_linear(a, (const float *)ly.fc_w, v.M, 4 * W, W, ly.fc_b, hbuf, 4 * W, F32_LIN_GELU, stream)))
            return rc;
        if ((rc = mpreid_gemm_f32_linear(hbuf, (const float *)ly.proj_w, v.M, W, 4 * W, ly.proj_b, x, W, F32_LIN_RES, stream)))
            return rc;
    }
    return image_head(cfg, w, x, (int64_t)L * W, B, y_cls, out, stream);
}

// fp32 LayerNorm for the backward sweep (towers.h; csrc/vit_grad.hip)
int vit_layernorm_f32(const float *x, int64_t rows, int W, const float *g, const float *b, float *out, hipStream_t stream) {
    hipLaunchKernelGGL(layernorm_kernel<0>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, x, rows, W, g, b, (void *)out,
                       (int64_t)W);
    LAUNCH_CHECK();
    return MPREID_OK;
}

// The forward LayerNorm and the head alone, for unit tests and tools (include/mpreid.h): the checks, then the launchers the
// towers call (vit_layernorm_f32: the instantiation ln_pre runs in place; block_layernorm: a block's GEMM operand)
extern "C" int mpreid_layernorm_f32(const float *x, int64_t rows, int width, const float *gamma, const float *beta, int form,
                                    void *out, mpreid_stream_t stream) {
    ARG_CHECK(x && gamma && beta && out && rows >= 0);
    ARG_CHECK(form >= 0 && form <= 2);
    const int rc = check_row_width("mpreid_layernorm_f32", width);
    if (rc) return rc;
    ARG_CHECK((((uintptr_t)x | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)out) & 15) == 0);
    ARG_CHECK(rows <= ((int64_t)1 << 31) - 256);   // block_layernorm's row count is an int
    if (rows == 0) return MPREID_OK;
    if (form == 0) return vit_layernorm_f32(x, rows, width, gamma, beta, (float *)out, (hipStream_t)stream);
    const bool split = form == 2;
    const BlockCtx ctx{(hipStream_t)stream, split, split ? 2 : 1, width, width / 64, 1, (int)rows};
    block_layernorm(ctx, x, (int)rows, gamma, beta, (_Float16 *)out);
    LAUNCH_CHECK();
    return MPREID_OK;
}

extern "C" int mpreid_tower_head_f32(const float *x, int64_t item_stride, const int32_t *row_of, int tokens, int batch, int width,
                                     int out_dim, const float *ln_g, const float *ln_b, const float *proj, const float *bn_scale,
                                     const float *bn_shift, const float *bnp_scale, const float *bnp_shift, float *y, float *out,
                                     int out_stride, int out_col, int ln_to_out, mpreid_stream_t stream) {
    ARG_CHECK(x && ln_g && ln_b && proj && y && out);
    ARG_CHECK((bn_scale != nullptr) == (bn_shift != nullptr) && (bnp_scale != nullptr) == (bnp_shift != nullptr));
    ARG_CHECK(batch >= 0 && batch <= 1 << 24 && tokens >= 1 && item_stride >= 0 && out_dim >= 1 && out_dim <= 1 << 20);
    const int rc = check_row_width("mpreid_tower_head_f32", width);
    if (rc) return rc;
    ARG_CHECK(out_col >= 0 && (int64_t)out_stride >= (int64_t)out_col + out_dim && (!ln_to_out || out_col >= width));
    ARG_CHECK(((uintptr_t)x & 15) == 0);
    ARG_CHECK((((uintptr_t)row_of | (uintptr_t)ln_g | (uintptr_t)ln_b | (uintptr_t)proj | (uintptr_t)bn_scale | (uintptr_t)bn_shift |
                (uintptr_t)bnp_scale | (uintptr_t)bnp_shift | (uintptr_t)y | (uintptr_t)out) & 3) == 0);
    if (batch == 0) return MPREID_OK;
    return tower_head(x, item_stride, row_of, tokens, batch, width, out_dim, ln_g, ln_b, proj, bn_scale, bn_shift, bnp_scale,
                      bnp_shift, y, out, out_stride, out_col, ln_to_out != 0, (hipStream_t)stream);
}

// the split mode's block and its parts for any tower (towers.h)
static BlockCtx split_ctx(const BlockShape &s, hipStream_t stream) { return BlockCtx{stream, true, 2, s.W, s.heads, s.B, s.L}; }
static AttnKind attn_kind(const BlockShape &s) { return s.causal ? ATTN_CAUSAL : ATTN_ALL_ROWS; }

int tower_block(const BlockShape &s, const mpreid_vit_layer &ly, float *x, _Float16 *a, float *qkv, _Float16 *hbuf, int Mpad,
                hipStream_t stream) {
    const BlockCtx ctx = split_ctx(s, stream);
    const int rc = block_attention_part(ctx, ly, x, a, qkv, s.M(), Mpad, attn_kind(s));
    return rc ? rc : block_mlp_part(ctx, ly, x, a, hbuf, s.M(), Mpad, nullptr, 0, nullptr, nullptr);
}

int tower_block_attention(const BlockShape &s, const mpreid_vit_layer &ly, const float *x, _Float16 *a, float *qkv, int Mpad,
                          hipStream_t stream) {
    return block_attention_part(split_ctx(s, stream), ly, x, a, qkv, s.M(), Mpad, attn_kind(s));
}

int tower_block_mid(const BlockShape &s, const mpreid_vit_layer &ly, float *x, _Float16 *a, int Mpad, hipStream_t stream) {
    return block_mid_part(split_ctx(s, stream), ly, x, a, s.M(), Mpad);
}

int tower_block_mlp_recompute(const BlockShape &s, const mpreid_vit_layer &ly, float *x, _Float16 *a, float *u, int Mpad,
                              hipStream_t stream) {
    return block_mlp_part(split_ctx(s, stream), ly, x, a, nullptr, s.M(), Mpad, nullptr, 0, nullptr, nullptr, u);
}
