// vit_grad.hip — the differentiation of the image tower (include/mpreid.h, "The image tower's gradient").  What is here:
// mpreid_vit_attention_backward, the unmasked attention gradient for 2 .. MPREID_VIT_MAX_TOKENS tokens.  The causal kernel of
// text_grad.hip keeps Q, K, V and dO of a head in LDS (146 KiB at 128 tokens) and cannot grow; this one makes two passes
// over a small workspace of row statistics and streams the other operand through LDS in 64-row blocks, so its LDS request
// does not depend on which operand is long.  No atomics: every sum has one fixed order, the same bits from run to run and
// for an image alone or inside a batch.
// Behind it: the transposing and column-sum kernels of the parameter gradients; the ONE differentiation of a residual block
// (block_mlp_backward / block_attention_backward, declared in towers.h), which mpreid_text_backward (csrc/text_grad.hip)
// calls with no parameter gradient and the causal attention kernel, and the sweep of this file with the kernels above; and
// mpreid_vit_backward / mpreid_vit_backward_moe: the checks and the per-call state in vit_backward_impl, then the kept
// forward, the head, the layer sweep and the embedding, one file-local function each.
#include "moe.h"
#include "towers.h"

namespace {

constexpr int VB_NW = 8;      // waves per workgroup = query rows (pass 1) / key rows (pass 2) of a workgroup's tile
constexpr int VB_BLK = 64;    // rows of the streamed operand per LDS block: one per lane
constexpr int VB_LD = 68;     // floats per LDS row: 64 + 4, so that the 16-byte reads of 16 consecutive rows cover all 64 banks

static int vb_lpad(int L) { return (L + VB_BLK - 1) / VB_BLK * VB_BLK; }
// pass 1: K and V block, the tile's Q and dO rows, per wave a strip of scores and a strip of dP over the padded row
static size_t vb_lds_rows(int L) { return ((size_t)2 * VB_BLK * VB_LD + 2 * VB_NW * VB_LD + (size_t)VB_NW * 2 * vb_lpad(L)) * sizeof(float); }
// pass 2: Q and dO block, the tile's K and V rows, per wave a strip of P and a strip of dS over one block
static size_t vb_lds_cols() { return ((size_t)2 * VB_BLK * VB_LD + 2 * VB_NW * VB_LD + (size_t)VB_NW * 2 * VB_BLK) * sizeof(float); }

// rows j0 .. j0 + 63 of one head of two [rows][ld] matrices -> two LDS blocks [64][VB_LD]; rows at or behind L are zeros
__device__ __forceinline__ void load_block_pair(const float *__restrict__ a, const float *__restrict__ b, int64_t lda, int64_t ldb,
                                                int j0, int L, float *__restrict__ As, float *__restrict__ Bs, int tid) {
    for (int idx = tid; idx < VB_BLK * 16; idx += 64 * VB_NW) {
        const int r = idx >> 4, c = (idx & 15) * 4;
        float4 va = make_float4(0.f, 0.f, 0.f, 0.f), vb = va;
        if (j0 + r < L) {
            va = *reinterpret_cast<const float4 *>(a + (int64_t)(j0 + r) * lda + c);
            vb = *reinterpret_cast<const float4 *>(b + (int64_t)(j0 + r) * ldb + c);
        }
        *reinterpret_cast<float4 *>(As + r * VB_LD + c) = va;
        *reinterpret_cast<float4 *>(Bs + r * VB_LD + c) = vb;
    }
}

// the same for one matrix
__device__ __forceinline__ void load_block(const float *__restrict__ a, int64_t lda, int j0, int L, float *__restrict__ As, int tid) {
    for (int idx = tid; idx < VB_BLK * 16; idx += 64 * VB_NW) {
        const int r = idx >> 4, c = (idx & 15) * 4;
        float4 va = make_float4(0.f, 0.f, 0.f, 0.f);
        if (j0 + r < L) va = *reinterpret_cast<const float4 *>(a + (int64_t)(j0 + r) * lda + c);
        *reinterpret_cast<float4 *>(As + r * VB_LD + c) = va;
    }
}

// Pass 1, one workgroup per (image, head, tile of 8 query rows), one wave per query row i.  K and V of the head stream
// through LDS in 64-key blocks, lane = key: s[j] = dot64(q_i, k_j) / 8 and dP[j] = dot64(dO_i, v_j) go to the wave's strips.
// Then the row's statistics: the maximum m, the first key j* that holds it, sum = sum_j exp(s[j] - m), r = dP[j*] and
// dot = sum_j P[j] (dP[j] - r) -- lane l adds the keys l, l + 64, ... in ascending order, then the butterfly 32 .. 1 -- are
// written to stats[(image * heads + head) * L + i] = (m, sum, r, dot), and dS[j] = P[j] ((dP[j] - r) - dot) replaces s[j] in
// the strip.  dS is taken about the row's strongest key, as in text_grad.hip: the same value in exact arithmetic (P sums
// to one), without the cancellation that costs a saturated row its digits.  K streams a second time, lane = feature:
// dQ[i] = sum_j dS[j] k_j / 8, j ascending in one fmaf chain.
__global__ __launch_bounds__(64 * VB_NW) void vit_attention_backward_rows_kernel(const float *__restrict__ qkv,
                                                                               const float *__restrict__ d_o, int L, int W,
                                                                               int heads, int tiles, float4 *__restrict__ stats,
                                                                               float *__restrict__ d_qkv) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *Ks = reinterpret_cast<float *>(smem);
    float *Vs = Ks + VB_BLK * VB_LD;
    float *Qs = Vs + VB_BLK * VB_LD;
    float *Gs = Qs + VB_NW * VB_LD;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lpad = (L + VB_BLK - 1) / VB_BLK * VB_BLK;
    float *strip_s = Gs + VB_NW * VB_LD + (size_t)wave * 2 * lpad;
    float *strip_dp = strip_s + lpad;

    const int tile = blockIdx.x % tiles, bh = blockIdx.x / tiles;
    const int b = bh / heads, h = bh - b * heads;
    const int64_t row0 = (int64_t)b * L;
    const int i = tile * VB_NW + wave;
    const bool active = i < L;   // (per wave)
    const float *kbase = qkv + row0 * 3 * W + W + h * 64;
    const float *vbase = kbase + W;
    float *qs = Qs + wave * VB_LD, *gs = Gs + wave * VB_LD;
    qs[lane] = active ? qkv[(row0 + i) * 3 * W + h * 64 + lane] : 0.f;
    gs[lane] = active ? d_o[(row0 + i) * W + h * 64 + lane] : 0.f;

    for (int j0 = 0; j0 < L; j0 += VB_BLK) {
        __syncthreads();   // the previous block has been read (first turn: nothing)
        load_block_pair(kbase, vbase, 3 * (int64_t)W, 3 * (int64_t)W, j0, L, Ks, Vs, tid);
        __syncthreads();   // (qs / gs of this wave are visible too)
        if (active && j0 + lane < L) {
            strip_s[j0 + lane] = dot64(qs, Ks + lane * VB_LD) * 0.125f;
            strip_dp[j0 + lane] = dot64(gs, Vs + lane * VB_LD);
        }
    }
    wave_lds_sync();
    if (active) {
        float m = strip_s[lane < L ? lane : 0];
        for (int j = lane + 64; j < L; j += 64) m = fmaxf(m, strip_s[j]);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
        int jstar = MPREID_VIT_MAX_TOKENS;
        float sum = 0.f;
        for (int j = lane; j < L; j += 64) {
            const float s = strip_s[j];
            if (s == m) jstar = min(jstar, j);
            sum += expf(s - m);
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) jstar = min(jstar, __shfl_xor(jstar, off, 64));
        sum = wave_bfly_add(sum);
        const float ref = strip_dp[jstar];
        float dot = 0.f;
        for (int j = lane; j < L; j += 64) dot = fmaf(__fdiv_rn(expf(strip_s[j] - m), sum), strip_dp[j] - ref, dot);
        dot = wave_bfly_add(dot);
        if (lane == 0) stats[(int64_t)bh * L + i] = make_float4(m, sum, ref, dot);
        for (int j = lane; j < L; j += 64)
            strip_s[j] = __fdiv_rn(expf(strip_s[j] - m), sum) * ((strip_dp[j] - ref) - dot);
    }
    wave_lds_sync();
    float acc = 0.f;
    for (int j0 = 0; j0 < L; j0 += VB_BLK) {
        __syncthreads();
        load_block(kbase, 3 * (int64_t)W, j0, L, Ks, tid);   // (V is not read again)
        __syncthreads();
        if (active) {
            const int n = min(VB_BLK, L - j0);
            for (int j = 0; j < n; ++j) acc = fmaf(strip_s[j0 + j], Ks[j * VB_LD + lane], acc);
        }
    }
    if (active) d_qkv[(row0 + i) * 3 * W + h * 64 + lane] = acc * 0.125f;
}

// Pass 2, one workgroup per (image, head, tile of 8 keys), one wave per key j.  Q and dO of the head stream through LDS in
// 64-row blocks, lane = query i: P[i][j] and dS[i][j] are rebuilt from the stored row statistics with the expressions of pass
// 1 (the score is the same fmaf chain: the same bits) and go to the wave's strips; then lane = feature:
// dK[j] = sum_i dS[i][j] q_i / 8 and dV[j] = sum_i P[i][j] dO_i, i ascending in one fmaf chain each across the blocks.
__global__ __launch_bounds__(64 * VB_NW) void vit_attention_backward_cols_kernel(const float *__restrict__ qkv,
                                                                               const float *__restrict__ d_o, int L, int W,
                                                                               int heads, int tiles, const float4 *__restrict__ stats,
                                                                               float *__restrict__ d_qkv) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *Qs = reinterpret_cast<float *>(smem);
    float *Gs = Qs + VB_BLK * VB_LD;
    float *Ks = Gs + VB_BLK * VB_LD;
    float *Vs = Ks + VB_NW * VB_LD;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float *strip_p = Vs + VB_NW * VB_LD + wave * 2 * VB_BLK;
    float *strip_ds = strip_p + VB_BLK;

    const int tile = blockIdx.x % tiles, bh = blockIdx.x / tiles;
    const int b = bh / heads, h = bh - b * heads;
    const int64_t row0 = (int64_t)b * L;
    const int j = tile * VB_NW + wave;
    const bool active = j < L;   // (per wave)
    const float *qbase = qkv + row0 * 3 * W + h * 64;
    const float *gbase = d_o + row0 * W + h * 64;
    float *ks = Ks + wave * VB_LD, *vs = Vs + wave * VB_LD;
    ks[lane] = active ? qbase[(int64_t)j * 3 * W + W + lane] : 0.f;
    vs[lane] = active ? qbase[(int64_t)j * 3 * W + 2 * W + lane] : 0.f;

    float dk = 0.f, dv = 0.f;
    for (int i0 = 0; i0 < L; i0 += VB_BLK) {
        __syncthreads();   // the previous block and the strips have been read
        load_block_pair(qbase, gbase, 3 * (int64_t)W, (int64_t)W, i0, L, Qs, Gs, tid);
        __syncthreads();
        if (active) {
            if (i0 + lane < L) {
                const float4 st = stats[(int64_t)bh * L + i0 + lane];   // (m, sum, r, dot) of query row i0 + lane
                const float sc = dot64(Qs + lane * VB_LD, ks) * 0.125f;
                const float p = __fdiv_rn(expf(sc - st.x), st.y);
                const float dp = dot64(Gs + lane * VB_LD, vs);
                strip_p[lane] = p;
                strip_ds[lane] = p * ((dp - st.z) - st.w);
            }
            wave_lds_sync();
            const int n = min(VB_BLK, L - i0);
            for (int r = 0; r < n; ++r) {
                dk = fmaf(strip_ds[r], Qs[r * VB_LD + lane], dk);
                dv = fmaf(strip_p[r], Gs[r * VB_LD + lane], dv);
            }
        }
    }
    if (active) {
        float *dst = d_qkv + (row0 + j) * 3 * W + h * 64 + lane;
        dst[W] = dk * 0.125f;
        dst[2 * W] = dv;
    }
}

size_t attn_bwd_ws_bytes(int64_t B, int L, int heads) { return align_up((size_t)B * heads * L * sizeof(float4), 256); }

int vit_attention_backward_check(int B, int L, int W, int heads) {
    const int shape = check_width_heads(W, heads);
    if (shape == SHAPE_HEAD_DIM) {
        mpreid_set_error("head dim must be 64 (width %d, heads %d)", W, heads);
        return MPREID_ERR_UNSUPPORTED;
    }
    if (shape != SHAPE_OK) {
        mpreid_set_error("unsupported width %d (a multiple of 128 up to 1024)", W);
        return MPREID_ERR_UNSUPPORTED;
    }
    if (L < 2 || L > MPREID_VIT_MAX_TOKENS) {
        mpreid_set_error("token count %d outside 2 .. %d (MPREID_VIT_MAX_TOKENS)", L, MPREID_VIT_MAX_TOKENS);
        return MPREID_ERR_UNSUPPORTED;
    }
    ARG_CHECK(B > 0);
    const int64_t tiles = (L + VB_NW - 1) / VB_NW;
    ARG_CHECK((int64_t)B * heads * tiles < (int64_t)1 << 31 && (int64_t)B * L * 3 * W < (int64_t)1 << 40);
    return MPREID_OK;
}

// d_qkv = the gradient of q | k | v; stats: B * heads * L float4 of workspace.  Shapes are checked by the caller.
int vit_attention_backward_launch(const float *qkv, const float *d_o, int B, int L, int W, int heads, float *d_qkv, void *stats,
                                  hipStream_t s) {
    const int tiles = (L + VB_NW - 1) / VB_NW;
    const size_t lds_rows = vb_lds_rows(L), lds_cols = vb_lds_cols();
    int rc = mpreid_dyn_lds(vit_attention_backward_rows_kernel, lds_rows);
    if (rc) return rc;
    if ((rc = mpreid_dyn_lds(vit_attention_backward_cols_kernel, lds_cols))) return rc;
    const dim3 grid((unsigned)((int64_t)B * heads * tiles));
    hipLaunchKernelGGL(vit_attention_backward_rows_kernel, grid, dim3(64 * VB_NW), lds_rows, s, qkv, d_o, L, W, heads, tiles,
                       (float4 *)stats, d_qkv);
    hipLaunchKernelGGL(vit_attention_backward_cols_kernel, grid, dim3(64 * VB_NW), lds_cols, s, qkv, d_o, L, W, heads, tiles,
                       (const float4 *)stats, d_qkv);
    LAUNCH_CHECK();
    return MPREID_OK;
}

}   // namespace

extern "C" size_t mpreid_vit_attention_backward_workspace_bytes(int batch, int tokens, int heads) {
    if (batch <= 0 || heads <= 0 || tokens < 2 || tokens > MPREID_VIT_MAX_TOKENS) return 0;
    return attn_bwd_ws_bytes(batch, tokens, heads);
}

extern "C" int mpreid_vit_attention_backward(const float *qkv, const float *d_o, int B, int L, int W, int heads, float *d_qkv,
                                             void *ws, size_t ws_bytes, mpreid_stream_t stream) {
    ARG_CHECK(qkv && d_o && d_qkv && B > 0);
    ARG_CHECK(((uintptr_t)qkv & 15) == 0 && ((uintptr_t)d_o & 15) == 0 && ((uintptr_t)d_qkv & 15) == 0);
    const int rc = vit_attention_backward_check(B, L, W, heads);
    if (rc) return rc;
    const size_t need = attn_bwd_ws_bytes(B, L, heads);
    if (!ws || ws_bytes < need) {
        mpreid_set_error("vit attention backward workspace too small: %zu < %zu", ws_bytes, need);
        return MPREID_ERR_WORKSPACE;
    }
    ARG_CHECK(((uintptr_t)ws & 15) == 0);
    return vit_attention_backward_launch(qkv, d_o, B, L, W, heads, d_qkv, ws, (hipStream_t)stream);
}

// =====================================================================================================================
// mpreid_vit_backward: the sweep over the layers and the parameter gradients
// =====================================================================================================================
namespace {

// dst[c][m] = op(src[row(m)][c]) for m < rows, 0 for rows <= m < rows_pad: the two operands of a weight gradient
// dW = dY^T X = (dY^T [N][Mpad]) . (X^T [K][Mpad])^T on the NT GEMM.  32 x 32 tiles through LDS ([32][33]: no bank conflict).
// MODE 0: src fp32 [rows][ld].  MODE 1: QuickGELU of it (the MLP's hidden layer from the FC1 pre-activation, the forward's
// expression).  MODE 2: src fp16 pairs [rows][hi(cols) | lo(cols)] (ld halfs per row) -> hi + lo, the value the forward's
// GEMM multiplied.  grp > 0: row(m) = (m / grp) * (grp + 1) + 1 + m % grp, the patch rows of a [B][grp + 1] token sequence.
template <int MODE>
__global__ __launch_bounds__(256) void transpose_pad_kernel(const void *__restrict__ src, int64_t rows, int cols, int64_t ld,
                                                            int grp, float *__restrict__ dst, int64_t rows_pad) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int64_t m0 = (int64_t)blockIdx.x * 32;
    const int c0 = blockIdx.y * 32;
    for (int r = ty; r < 32; r += 8) {
        const int64_t m = m0 + r;
        const int c = c0 + tx;
        float v = 0.f;
        if (m < rows && c < cols) {
            const int64_t sr = grp > 0 ? (m / grp) * (grp + 1) + 1 + m % grp : m;
            if (MODE == 2) {
                const _Float16 *p = reinterpret_cast<const _Float16 *>(src) + sr * ld;
                v = (float)p[c] + (float)p[cols + c];
            } else {
                v = reinterpret_cast<const float *>(src)[sr * ld + c];
                if (MODE == 1) v = __fdiv_rn(v, 1.0f + expf(-1.702f * v));
            }
        }
        tile[r][tx] = v;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int c = c0 + r;
        const int64_t m = m0 + tx;
        if (c < cols && m < rows_pad) dst[(int64_t)c * rows_pad + m] = tile[tx][r];
    }
}

int launch_transpose(int mode, const void *src, int64_t rows, int cols, int64_t ld, int grp, float *dst, int64_t rows_pad,
                     hipStream_t s) {
    const dim3 grid((unsigned)((rows_pad + 31) / 32), (unsigned)((cols + 31) / 32));
    if (mode == 0)
        hipLaunchKernelGGL(transpose_pad_kernel<0>, grid, dim3(256), 0, s, src, rows, cols, ld, grp, dst, rows_pad);
    else if (mode == 1)
        hipLaunchKernelGGL(transpose_pad_kernel<1>, grid, dim3(256), 0, s, src, rows, cols, ld, grp, dst, rows_pad);
    else
        hipLaunchKernelGGL(transpose_pad_kernel<2>, grid, dim3(256), 0, s, src, rows, cols, ld, grp, dst, rows_pad);
    LAUNCH_CHECK();
    return MPREID_OK;
}

// Column sums over the rows, for bias / beta gradients (sum_m dy[m][c]) and gamma gradients (sum_m dy[m][c] xhat[m][c]).
// Fixed order: the rows are cut into pieces of CS_ROWS; a thread adds its column over one piece, rows ascending; the pieces'
// partial sums are then added in ascending order by colsum_final_kernel.  Every operation is a single rounded fp32 operation
// (no fused multiply-add), so the sums can be restated bit for bit on the host.
constexpr int CS_ROWS = 128;

// (mean, 1 / sigma) of every row of x (biased variance, eps 1e-5), one wave per row: lane l adds the elements l, l + 64, ...
// ascending, then the butterfly 32 .. 1
__global__ __launch_bounds__(256) void row_stats_kernel(const float *__restrict__ x, int64_t rows, int W, int64_t ld,
                                                        float2 *__restrict__ st) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float *xr = x + row * ld;
    float s = 0.f;
    for (int k = lane; k < W; k += 64) s = __fadd_rn(s, xr[k]);
    const float mean = __fdiv_rn(wave_bfly_add(s), (float)W);
    float q = 0.f;
    for (int k = lane; k < W; k += 64) {
        const float d = __fsub_rn(xr[k], mean);
        q = __fadd_rn(q, __fmul_rn(d, d));
    }
    // (sqrtf: the correctly rounded square root, so that the host can restate the bits; __fsqrt_rn is the 1-ulp instruction)
    const float rstd = __fdiv_rn(1.0f, sqrtf(__fadd_rn(__fdiv_rn(wave_bfly_add(q), (float)W), 1e-5f)));
    if (lane == 0) st[row] = make_float2(mean, rstd);
}

// grid (ceil(cols / 256), pieces); psum / psumx [pieces][cols], either may be NULL (psumx needs x and st)
__global__ __launch_bounds__(256) void colsum_partial_kernel(const float *__restrict__ dy, int64_t ld, const float *__restrict__ x,
                                                             int64_t ldx, const float2 *__restrict__ st, int64_t rows, int cols,
                                                             float *__restrict__ psum, float *__restrict__ psumx) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= cols) return;
    const int64_t r0 = (int64_t)blockIdx.y * CS_ROWS;
    const int64_t r1 = r0 + CS_ROWS < rows ? r0 + CS_ROWS : rows;
    float s = 0.f, sx = 0.f;
    for (int64_t r = r0; r < r1; ++r) {
        const float d = dy[r * ld + c];
        s = __fadd_rn(s, d);
        if (psumx) {
            const float2 t = st[r];
            sx = __fadd_rn(sx, __fmul_rn(d, __fmul_rn(__fsub_rn(x[r * ldx + c], t.x), t.y)));
        }
    }
    if (psum) psum[(int64_t)blockIdx.y * cols + c] = s;
    if (psumx) psumx[(int64_t)blockIdx.y * cols + c] = sx;
}

__global__ __launch_bounds__(256) void colsum_final_kernel(const float *__restrict__ psum, const float *__restrict__ psumx,
                                                           int pieces, int cols, float *__restrict__ out_sum,
                                                           float *__restrict__ out_sumx) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= cols) return;
    if (out_sum) {
        float s = psum[c];
        for (int p = 1; p < pieces; ++p) s = __fadd_rn(s, psum[(int64_t)p * cols + c]);
        out_sum[c] = s;
    }
    if (out_sumx) {
        float s = psumx[c];
        for (int p = 1; p < pieces; ++p) s = __fadd_rn(s, psumx[(int64_t)p * cols + c]);
        out_sumx[c] = s;
    }
}

int64_t colsum_pieces(int64_t rows) { return (rows + CS_ROWS - 1) / CS_ROWS; }
// the reduction's workspace: two partial arrays [pieces][cols], then the row statistics
size_t colsum_part_bytes(int64_t rows, int64_t cols) { return align_up((size_t)colsum_pieces(rows) * cols * 4, 256); }
size_t colsum_ws_bytes(int64_t rows, int64_t cols) { return 2 * colsum_part_bytes(rows, cols) + align_up((size_t)rows * 8, 256); }

// out_sum[c] = sum_m dy[m][c]; out_sumx[c] = sum_m dy[m][c] xhat(x)[m][c] (x rows are `cols` wide); either may be NULL
int launch_colsum(const float *dy, int64_t ld, const float *x, int64_t ldx, int64_t rows, int cols, float *out_sum,
                  float *out_sumx, void *ws, hipStream_t s) {
    if (!out_sum && !out_sumx) return MPREID_OK;
    const size_t pb = colsum_part_bytes(rows, cols);
    float *psum = (float *)ws, *psumx = (float *)((char *)ws + pb);
    float2 *st = (float2 *)((char *)ws + 2 * pb);
    const int pieces = (int)colsum_pieces(rows);
    if (out_sumx) {
        hipLaunchKernelGGL(row_stats_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, x, rows, cols, ldx, st);
        LAUNCH_CHECK();
    }
    const dim3 grid((unsigned)((cols + 255) / 256), (unsigned)pieces);
    hipLaunchKernelGGL(colsum_partial_kernel, grid, dim3(256), 0, s, dy, ld, x, ldx, st, rows, cols, out_sum ? psum : nullptr,
                       out_sumx ? psumx : nullptr);
    hipLaunchKernelGGL(colsum_final_kernel, dim3(grid.x), dim3(256), 0, s, psum, psumx, pieces, cols, out_sum, out_sumx);
    LAUNCH_CHECK();
    return MPREID_OK;
}

// The head's seed: hy[b][k] = d_f[b][k] + sum_o d_f_proj[b][o] proj[k][o] (o ascending in one fmaf chain); a NULL seed is zero
__global__ __launch_bounds__(256) void vit_head_seed_kernel(const float *__restrict__ d_f, const float *__restrict__ d_fp,
                                                            const float *__restrict__ proj, int B, int W, int out_dim,
                                                            float *__restrict__ hy) {
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gid >= (int64_t)B * W) return;
    const int b = (int)(gid / W), k = (int)(gid % W);
    float acc = 0.f;
    if (d_fp)
        for (int o = 0; o < out_dim; ++o) acc = fmaf(d_fp[(int64_t)b * out_dim + o], proj[(int64_t)k * out_dim + o], acc);
    hy[gid] = d_f ? d_f[gid] + acc : acc;
}

// dx[b * L][:] += add[b][:]: a seed on the CLS rows
__global__ __launch_bounds__(256) void add_cls_rows_kernel(const float *__restrict__ add, int B, int L, int W, float *__restrict__ dx) {
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gid >= (int64_t)B * W) return;
    const int b = (int)(gid / W), k = (int)(gid % W);
    dx[(int64_t)b * L * W + k] += add[gid];
}

// The backward call's workspace: the forward's regions first (f.hbuf doubles as the fp32 FC1 pre-activation: the same 16 W
// bytes per row), then what the sweep keeps
struct VitGradLayout {
    VitLayout f;
    int64_t Mp4, Bp4, tw;
    size_t tok;
    SweepRegions r;   // xs, dx, dh, t, dqkv (towers.h)
    size_t aot, at, bt, stats, red, small, total;
    // an MoE tower's share, behind the dense sweep's: the routing of block 0, its logits, d_w summed over the MoE blocks,
    // d_logits, and the routed MLP's gradient workspace (tables of the dispatch, hidden, y, u)
    MoeGradLayout mg;
    size_t sel, rw, logits, d_w, d_logits, moe;
};

VitGradLayout vit_grad_layout(const mpreid_vit_cfg *c, int B, const mpreid_vit_moe *moe = nullptr) {
    VitGradLayout v{};
    v.f = vit_layout(c, B);
    const size_t W = (size_t)c->width;
    const size_t row = (size_t)v.f.Mpad * W * 4;   // one fp32 [Mpad][W] buffer
    v.Mp4 = (int64_t)align_up((size_t)v.f.M, 4);   // the row count of a transposed operand: the GEMM's K, a multiple of 4
    v.Bp4 = (int64_t)align_up((size_t)B, 4);
    v.tw = 4 * (int64_t)W;                         // the widest matrix that is transposed
    if (v.f.Kp > v.tw) v.tw = v.f.Kp;
    if (c->out_dim > v.tw) v.tw = c->out_dim;
    WsCursor take{v.f.total};
    v.tok = take(row);                             // the embedded sequence, ln_pre's input
    v.r = take_sweep_regions(take, row, c->layers);
    v.aot = take((size_t)v.Mp4 * W * 4);           // the attention output, transposed [W][Mp4]
    v.at = take((size_t)v.Mp4 * v.tw * 4);         // dY^T
    v.bt = take((size_t)v.Mp4 * v.tw * 4);         // X^T
    v.stats = take(attn_bwd_ws_bytes(B, v.f.L, c->heads));
    size_t red = colsum_ws_bytes(v.f.M, 4 * (int64_t)W);
    const size_t red_pos = colsum_ws_bytes(B, (int64_t)v.f.L * (int64_t)W);
    v.red = take(red > red_pos ? red : red_pos);   // the column reductions' partial sums and row statistics
    v.small = take(4 * align_up((size_t)B * W * 4, 256));   // CLS rows of x, the head's seed, f, the CLS rows' gradient
    if (moe) {
        const size_t E = (size_t)moe->num_experts, K = (size_t)moe->top_k, M = (size_t)v.f.M;
        v.mg = moe_grad_layout((int64_t)M, c->width, moe->num_experts, moe->top_k);
        v.sel = take(M * K * 4);
        v.rw = take(M * K * 4);
        v.logits = take(M * E * 4);
        v.d_w = take(M * K * 4);
        v.d_logits = take(M * E * 4);
        v.moe = take(v.mg.total);
    }
    v.total = take.off;
    return v;
}

int vit_backward_check_cfg(const mpreid_vit_cfg *cfg) {
    const int rc = vit_check_cfg(cfg);
    if (rc) return rc;
    if (cfg->precision != MPREID_VIT_SPLIT || cfg->layers < 1) {
        mpreid_set_error("the image tower's backward runs the dense tower in the split precision with at least one layer "
                         "(precision %d, layers %d)", cfg->precision, cfg->layers);
        return MPREID_ERR_UNSUPPORTED;
    }
    return vit_attention_backward_check(1, cfg->h_res * cfg->w_res + 1, cfg->width, cfg->heads);
}

}   // namespace

extern "C" int mpreid_transpose_pad_f32(const float *src, int64_t rows, int cols, float *dst, int64_t rows_pad,
                                        mpreid_stream_t stream) {
    ARG_CHECK(src && dst && rows > 0 && cols > 0 && rows_pad >= rows);
    ARG_CHECK(rows_pad < (int64_t)1 << 31 && cols <= 65535 * 32);
    return launch_transpose(0, src, rows, cols, cols, 0, dst, rows_pad, (hipStream_t)stream);
}

extern "C" size_t mpreid_colsum_workspace_bytes(int64_t rows, int cols) {
    if (rows <= 0 || cols <= 0) return 0;
    return colsum_ws_bytes(rows, cols);
}

extern "C" int mpreid_colsum_f32(const float *dy, const float *x, int64_t rows, int cols, float *out_sum, float *out_sumx,
                                 void *ws, size_t ws_bytes, mpreid_stream_t stream) {
    ARG_CHECK(dy && rows > 0 && cols > 0 && (out_sum || out_sumx) && (x || !out_sumx));
    ARG_CHECK(colsum_pieces(rows) <= 65535);
    const size_t need = colsum_ws_bytes(rows, cols);
    if (!ws || ws_bytes < need) {
        mpreid_set_error("colsum workspace too small: %zu < %zu", ws_bytes, need);
        return MPREID_ERR_WORKSPACE;
    }
    ARG_CHECK(((uintptr_t)ws & 255) == 0);
    return launch_colsum(dy, cols, x, cols, rows, cols, out_sum, out_sumx, ws, (hipStream_t)stream);
}

extern "C" size_t mpreid_vit_backward_workspace_bytes(const mpreid_vit_cfg *cfg, int batch) {
    if (!cfg || batch <= 0 || vit_backward_check_cfg(cfg)) return 0;
    return vit_grad_layout(cfg, batch).total;
}

// =====================================================================================================================
// The one differentiation of a residual block (towers.h): the text tower's sweep (csrc/text_grad.hip, no parameter gradient)
// and the image towers' below call these two halves.  A NULL member of g launches nothing and touches no buffer.
// =====================================================================================================================
// dW [n][k] = sum_m dY[m][n] X[m][k]: c.at = dY^T and c.bt = X^T hold the operands
static int wgrad(const BlockGrad &c, float *out, int n, int k) {
    return mpreid_gemm_f32_linear(c.at, c.bt, n, k, (int)c.Mp4, nullptr, out, k, F32_LIN, c.stream);
}

int block_mlp_backward(const BlockGrad &c, const mpreid_vit_layer &ly, const mpreid_text_layer_t &lt,
                       const mpreid_vit_layer_grads &g) {
    const int W = c.s.W, M = c.s.M();
    hipStream_t stream = c.stream;
    int rc;
    if ((rc = tower_block_mlp_recompute(c.s, ly, c.x, c.a, c.u, c.Mpad, stream))) return rc;   // x = x_mid, a = ln_2(x_mid)
    if (g.proj_w) {   // X = quickgelu(u), the fp32 value the forward's hidden pair is split from
        if ((rc = launch_transpose(0, c.dx, M, W, W, 0, c.at, c.Mp4, stream))) return rc;
        if ((rc = launch_transpose(1, c.u, M, 4 * W, 4 * W, 0, c.bt, c.Mp4, stream))) return rc;
        if ((rc = wgrad(c, g.proj_w, W, 4 * W))) return rc;
    }
    if ((rc = launch_colsum(c.dx, W, nullptr, 0, M, W, g.proj_b, nullptr, c.red, stream))) return rc;
    if ((rc = mpreid_gemm_f32_linear(c.dx, lt.proj_t, M, 4 * W, W, nullptr, c.dh, 4 * W, F32_LIN, stream))) return rc;
    if ((rc = launch_quickgelu_backward(c.u, c.dh, (int64_t)M * W, stream))) return rc;   // dh = d/du; M * 4W / 4 float4
    if (g.fc_w) {
        if ((rc = launch_transpose(0, c.dh, M, 4 * W, 4 * W, 0, c.at, c.Mp4, stream))) return rc;
        if ((rc = launch_transpose(2, c.a, M, W, 2 * W, 0, c.bt, c.Mp4, stream))) return rc;
        if ((rc = wgrad(c, g.fc_w, 4 * W, W))) return rc;
    }
    if ((rc = launch_colsum(c.dh, 4 * W, nullptr, 0, M, 4 * W, g.fc_b, nullptr, c.red, stream))) return rc;
    return mpreid_gemm_f32_linear(c.dh, lt.fc_t, M, W, 4 * W, nullptr, c.t, W, F32_LIN, stream);
}

int block_attention_backward(const BlockGrad &c, const mpreid_vit_layer &ly, const mpreid_text_layer_t &lt, const float *xl,
                             const mpreid_vit_layer_grads &g) {
    const int W = c.s.W, M = c.s.M();
    hipStream_t stream = c.stream;
    int rc;
    if ((rc = launch_colsum(c.t, W, c.x, W, M, W, g.ln2_b, g.ln2_g, c.red, stream))) return rc;
    if ((rc = launch_layernorm_backward(c.x, c.t, ly.ln2_g, M, W, true, c.dx, stream))) return rc;   // dx = d/dx_mid
    if (g.out_proj_w) {
        if ((rc = launch_transpose(0, c.dx, M, W, W, 0, c.at, c.Mp4, stream))) return rc;
        if ((rc = mpreid_gemm_f32_linear(c.at, c.aot, W, W, (int)c.Mp4, nullptr, g.out_proj_w, W, F32_LIN, stream))) return rc;
    }
    if ((rc = launch_colsum(c.dx, W, nullptr, 0, M, W, g.out_proj_b, nullptr, c.red, stream))) return rc;
    if ((rc = mpreid_gemm_f32_linear(c.dx, lt.out_proj_t, M, W, W, nullptr, c.t, W, F32_LIN, stream))) return rc;
    if ((rc = c.s.causal ? launch_causal_attention_backward(c.qkv, c.t, c.s.B, c.s.L, W, c.s.heads, c.dqkv, stream)
                         : vit_attention_backward_launch(c.qkv, c.t, c.s.B, c.s.L, W, c.s.heads, c.dqkv, c.stats, stream)))
        return rc;
    if (g.in_proj_w) {
        if ((rc = vit_layernorm_f32(xl, M, W, ly.ln1_g, ly.ln1_b, c.t, stream))) return rc;   // the fp32 value in_proj's pair was split from
        if ((rc = launch_transpose(0, c.dqkv, M, 3 * W, 3 * W, 0, c.at, c.Mp4, stream))) return rc;
        if ((rc = launch_transpose(0, c.t, M, W, W, 0, c.bt, c.Mp4, stream))) return rc;
        if ((rc = wgrad(c, g.in_proj_w, 3 * W, W))) return rc;
    }
    if ((rc = launch_colsum(c.dqkv, 3 * W, nullptr, 0, M, 3 * W, g.in_proj_b, nullptr, c.red, stream))) return rc;
    if ((rc = mpreid_gemm_f32_linear(c.dqkv, lt.in_proj_t, M, W, 3 * W, nullptr, c.t, W, F32_LIN, stream))) return rc;
    if ((rc = launch_colsum(c.t, W, xl, W, M, W, g.ln1_b, g.ln1_g, c.red, stream))) return rc;
    return launch_layernorm_backward(xl, c.t, ly.ln1_g, M, W, true, c.dx, stream);   // dx = d/dx_l
}

// =====================================================================================================================
// The sweep of both image towers.  moe == nullptr: the dense tower.  Otherwise blocks l < moe->moe_layers (at least one) carry
// the routed MLP: their MLP half goes through csrc/moe_grad.hip, everything else through the same code as a dense block's.
// =====================================================================================================================
namespace {

// dx[:, 0] += d_f_last
int seed_f_last(const BlockGrad &c, const float *d_f_last) {
    hipLaunchKernelGGL(add_cls_rows_kernel, dim3((unsigned)(((int64_t)c.s.B * c.s.W + 255) / 256)), dim3(256), 0, c.stream, d_f_last,
                       c.s.B, c.s.L, c.s.W, c.dx);
    LAUNCH_CHECK();
    return MPREID_OK;
}

// the forward, keeping the embedded sequence and every x_l
int vit_backward_forward(const BlockGrad &c, const mpreid_vit_cfg *cfg, const mpreid_vit_weights *w, const mpreid_vit_moe *moe,
                         const mpreid_image_in &in, const float *cv_emb, const VitGradLayout &v, char *base) {
    const int W = c.s.W, M = c.s.M(), n_moe = moe ? moe->moe_layers : 0;
    float *tok = (float *)(base + v.tok), *xs = (float *)(base + v.r.xs);
    int rc;
    if ((rc = vit_embed_tokens(cfg, w, in, c.s.B, cv_emb, v.f, (_Float16 *)(base + v.f.patches), tok, true, c.stream)))
        return rc;
    if ((rc = vit_layernorm_f32(tok, M, W, w->ln_pre_g, w->ln_pre_b, c.x, c.stream))) return rc;
    for (int l = 0; l < cfg->layers; ++l) {
        const mpreid_vit_layer &ly = w->layers[l];
        HIP_TRY(hipMemcpyAsync(xs + l * (size_t)c.Mpad * W, c.x, (size_t)M * W * 4, hipMemcpyDeviceToDevice, c.stream));
        if (l >= n_moe) {
            if ((rc = tower_block(c.s, ly, c.x, c.a, c.qkv, (_Float16 *)(base + v.f.hbuf), c.Mpad, c.stream))) return rc;
            continue;
        }
        // an MoE block, launch for launch what mpreid_vit_forward_moe runs; block 0 keeps its routing and logits
        if ((rc = tower_block_attention(c.s, ly, c.x, c.a, c.qkv, c.Mpad, c.stream))) return rc;
        if ((rc = tower_block_mid(c.s, ly, c.x, c.a, c.Mpad, c.stream))) return rc;
        if (l == 0) {
            int32_t *sel = (int32_t *)(base + v.sel);
            float *rw = (float *)(base + v.rw);
            if ((rc = moe_route_launch(c.x, M, W, ly.ln2_g, ly.ln2_b, moe->layers[0].gate_w, moe->num_experts, moe->top_k, sel, rw,
                                       (float *)(base + v.logits), c.stream)))
                return rc;
            if ((rc = moe_dispatch_launch(sel, rw, v.mg.fwd, base + v.moe, c.stream))) return rc;
        }
        if ((rc = moe_mlp_launch(c.a, v.mg.fwd, &moe->layers[l], c.x, base + v.moe, c.stream))) return rc;
    }
    return MPREID_OK;
}

// The head at the CLS rows, f = ln_post(x[:, 0]), f_proj = f @ proj: the gradients of proj and ln_post; dx = the seed of the
// sweep.  small: CLS rows of x, the head's seed, f, the CLS rows' gradient
int vit_backward_head(const BlockGrad &c, const mpreid_vit_weights *w, const mpreid_vit_grads *grads, const float *d_f,
                      const float *d_f_proj, int od, int64_t Bp4, float *small) {
    const int B = c.s.B, W = c.s.W;
    hipStream_t stream = c.stream;
    const size_t sb = align_up((size_t)B * W * 4, 256) / 4, rowb = (size_t)W * 4, seqb = rowb * c.s.L;
    float *xc = small, *hy = small + sb, *fb = small + 2 * sb, *dxc = small + 3 * sb;
    int rc;
    HIP_TRY(hipMemcpy2DAsync(xc, rowb, c.x, seqb, rowb, (size_t)B, hipMemcpyDeviceToDevice, stream));
    hipLaunchKernelGGL(vit_head_seed_kernel, dim3((unsigned)(((int64_t)B * W + 255) / 256)), dim3(256), 0, stream, d_f, d_f_proj,
                       w->proj, B, W, od, hy);
    LAUNCH_CHECK();
    if (grads && grads->proj) {
        if (d_f_proj) {
            if ((rc = vit_layernorm_f32(xc, B, W, w->ln_post_g, w->ln_post_b, fb, stream))) return rc;
            if ((rc = launch_transpose(0, fb, B, W, W, 0, c.at, Bp4, stream))) return rc;
            if ((rc = launch_transpose(0, d_f_proj, B, od, od, 0, c.bt, Bp4, stream))) return rc;
            if ((rc = mpreid_gemm_f32_linear(c.at, c.bt, W, od, (int)Bp4, nullptr, grads->proj, od, F32_LIN, stream))) return rc;
        } else {
            HIP_TRY(hipMemsetAsync(grads->proj, 0, (size_t)W * od * 4, stream));
        }
    }
    if (grads && (rc = launch_colsum(hy, W, xc, W, B, W, grads->ln_post_b, grads->ln_post_g, c.red, stream))) return rc;
    if ((rc = launch_layernorm_backward(xc, hy, w->ln_post_g, B, W, false, dxc, stream))) return rc;
    HIP_TRY(hipMemsetAsync(c.dx, 0, (size_t)c.s.M() * W * 4, stream));
    HIP_TRY(hipMemcpy2DAsync(c.dx, seqb, dxc, rowb, rowb, (size_t)B, hipMemcpyDeviceToDevice, stream));
    return MPREID_OK;
}

// The layers, last to first: dx = d/dx_layers -> dx = d/dx_0.  An MoE block (l < moe->moe_layers) keeps its own MLP half:
// x_{l+1} = x_mid + sum_e w_e expert_e(ln_2(x_mid)): t = d/dh through the experts, d_w summed over the MoE blocks
int vit_backward_layers(const BlockGrad &c, int layers, const mpreid_vit_weights *w, const mpreid_vit_weights_t *wt,
                        const mpreid_vit_grads *grads, const mpreid_vit_moe *moe, const mpreid_vit_moe_t *moe_t, float aux_coef,
                        float *d_gate_w, float *l_aux_out, const float *d_f_last, const VitGradLayout &v, char *base) {
    const int W = c.s.W, M = c.s.M(), n_moe = moe ? moe->moe_layers : 0, E = moe ? moe->num_experts : 0, K = moe ? moe->top_k : 0;
    hipStream_t stream = c.stream;
    const mpreid_vit_layer_grads none{};
    // the MoE share (untouched offsets of a dense tower are never used)
    int32_t *sel = (int32_t *)(base + v.sel);
    float *d_w = (float *)(base + v.d_w), *d_logits = (float *)(base + v.d_logits);
    char *mws = base + v.moe;
    int rc;
    for (int l = layers - 1; l >= 0; --l) {
        const mpreid_vit_layer &ly = w->layers[l];
        const mpreid_vit_layer_grads &g = grads ? grads->layers[l] : none;
        const float *xl = (const float *)(base + v.r.xs) + l * (size_t)c.Mpad * W;
        HIP_TRY(hipMemcpyAsync(c.x, xl, (size_t)M * W * 4, hipMemcpyDeviceToDevice, stream));
        if ((rc = tower_block_attention(c.s, ly, c.x, c.a, c.qkv, c.Mpad, stream))) return rc;
        if (g.out_proj_w && (rc = launch_transpose(2, c.a, M, W, 2 * W, 0, c.aot, c.Mp4, stream))) return rc;
        if (l >= n_moe) {
            if ((rc = block_mlp_backward(c, ly, wt->layers[l], g))) return rc;
        } else {
            if ((rc = tower_block_mid(c.s, ly, c.x, c.a, c.Mpad, stream))) return rc;   // x = x_mid, a = ln_2(x_mid)
            if ((rc = moe_mlp_backward_launch(c.a, sel, v.mg, &moe->layers[l], &moe_t->layers[l], c.dx, c.t, d_w, l != n_moe - 1, mws,
                                              stream)))
                return rc;
            if (l == 0) {   // every MoE block has added to d_w: the router, its gate, and the gate's share of d/dh
                if ((rc = moe_route_backward_ws((const float *)(base + v.logits), sel, (const float *)(base + v.rw), d_w, M, E, K,
                                                aux_coef, d_logits, l_aux_out, (const int *)(mws + v.mg.fwd.meta) + MOE_META_COUNTS,
                                                mws + v.mg.cnt_blk, stream)))
                    return rc;
                if (d_gate_w) {   // d gate = d_logits^T . h, h the fp32 LayerNorm output the router saw
                    if ((rc = vit_layernorm_f32(c.x, M, W, ly.ln2_g, ly.ln2_b, c.dh, stream))) return rc;
                    if ((rc = launch_transpose(0, d_logits, M, E, E, 0, c.at, c.Mp4, stream))) return rc;
                    if ((rc = launch_transpose(0, c.dh, M, W, W, 0, c.bt, c.Mp4, stream))) return rc;
                    if ((rc = wgrad(c, d_gate_w, E, W))) return rc;
                }
                if ((rc = moe_gate_dh_launch(d_logits, moe->layers[0].gate_w, M, W, E, c.t, stream))) return rc;
            }
        }
        if ((rc = block_attention_backward(c, ly, wt->layers[l], xl, g))) return rc;
        // the dense tower's f_last is the CLS row of the last block's input
        if (!moe && l == layers - 1 && d_f_last && (rc = seed_f_last(c, d_f_last))) return rc;
    }
    return MPREID_OK;
}

// ln_pre, then the embedding: tokens = [class_emb + cv_emb | conv1(patches)] + pos_emb
int vit_backward_embed(const BlockGrad &c, const mpreid_vit_weights *w, const mpreid_vit_grads *grads, float *d_tokens,
                       const VitGradLayout &v, char *base) {
    const VitLayout &f = v.f;
    const int B = c.s.B, W = c.s.W, L = c.s.L, M = c.s.M();
    hipStream_t stream = c.stream;
    const float *tok = (const float *)(base + v.tok);
    const size_t rowb = (size_t)W * 4, seqb = rowb * L;
    int rc;
    if (grads && (rc = launch_colsum(c.dx, W, tok, W, M, W, grads->ln_pre_b, grads->ln_pre_g, c.red, stream))) return rc;
    const bool need_tok = d_tokens || (grads && (grads->conv_w || grads->class_emb || grads->pos_emb || grads->cv_emb));
    if (!need_tok) return MPREID_OK;
    float *dtok = d_tokens ? d_tokens : c.t;
    if ((rc = launch_layernorm_backward(tok, c.dx, w->ln_pre_g, M, W, false, dtok, stream))) return rc;
    if (!grads) return MPREID_OK;
    if (grads->cv_emb)
        HIP_TRY(hipMemcpy2DAsync(grads->cv_emb, rowb, dtok, seqb, rowb, (size_t)B, hipMemcpyDeviceToDevice, stream));
    if ((rc = launch_colsum(dtok, (int64_t)L * W, nullptr, 0, B, W, grads->class_emb, nullptr, c.red, stream))) return rc;
    if ((rc = launch_colsum(dtok, (int64_t)L * W, nullptr, 0, B, L * W, grads->pos_emb, nullptr, c.red, stream))) return rc;
    if (grads->conv_w) {   // over the B * P patch rows; X = the patch pairs the forward's GEMM multiplied
        const int64_t MP = (int64_t)B * f.P, MP4 = (int64_t)align_up((size_t)MP, 4);
        if ((rc = launch_transpose(0, dtok, MP, W, W, f.P, c.at, MP4, stream))) return rc;
        if ((rc = launch_transpose(2, base + f.patches, MP, f.Kp, 2 * (int64_t)f.Kp, 0, c.bt, MP4, stream))) return rc;
        if ((rc = mpreid_gemm_f32_linear(c.at, c.bt, W, f.Kp, (int)MP4, nullptr, grads->conv_w, f.Kp, F32_LIN, stream))) return rc;
    }
    return MPREID_OK;
}

// Both entry points: every refusal in their one order, all before anything is launched; then the per-call state (layout,
// BlockGrad) and the five steps above
int vit_backward_impl(const mpreid_vit_cfg *cfg, const mpreid_vit_weights *w, const mpreid_vit_weights_t *wt,
                      const mpreid_vit_moe *moe, const mpreid_vit_moe_t *moe_t, float aux_coef, float *d_gate_w, float *l_aux_out,
                      const mpreid_image_in *img, int B, const float *cv_emb, const float *d_f_last, const float *d_f,
                      const float *d_f_proj, const mpreid_vit_grads *grads, float *d_tokens, void *ws, size_t ws_bytes,
                      mpreid_stream_t stream_) {
    int rc = vit_backward_check_cfg(cfg);
    if (rc) return rc;
    const int n_moe = moe ? moe->moe_layers : 0;
    if (moe) {
        if ((rc = vit_check_moe_call(cfg, moe, B))) return rc;
        if (n_moe < 1) {
            mpreid_set_error("mpreid_vit_backward_moe needs at least one MoE block (moe_layers %d): a tower without one is the "
                             "dense tower of mpreid_vit_backward", n_moe);
            return MPREID_ERR_UNSUPPORTED;
        }
        ARG_CHECK(moe_t && moe_t->layers);
        for (int l = 0; l < n_moe; ++l) {
            const mpreid_moe_layer_t &t = moe_t->layers[l];
            ARG_CHECK(t.fc_t && t.proj_t && (((uintptr_t)t.fc_t | (uintptr_t)t.proj_t) & 15) == 0);
        }
        // (asked of moe_grad.hip: this file is compiled with -ffinite-math-only, which folds any test for NaN or infinity away)
        ARG_CHECK(moe_coef_is_finite(aux_coef));
        ARG_CHECK((((uintptr_t)d_gate_w | (uintptr_t)l_aux_out) & 3) == 0);
    }
    mpreid_image_in in;
    if ((rc = mpreid_check_image_in(img, &in))) return rc;
    ARG_CHECK(w && wt && B > 0 && w->layers && wt->layers);
    ARG_CHECK(w->conv_w && w->class_emb && w->pos_emb && w->ln_pre_g && w->ln_pre_b && w->ln_post_g && w->ln_post_b && w->proj);
    ARG_CHECK(!grads || grads->layers);
    ARG_CHECK((((uintptr_t)cv_emb | (uintptr_t)d_f_last | (uintptr_t)d_f | (uintptr_t)d_f_proj) & 3) == 0 &&
              ((uintptr_t)d_tokens & 15) == 0);
    const VitGradLayout v = vit_grad_layout(cfg, B, moe);
    ARG_CHECK((int64_t)B * v.f.L <= ((int64_t)1 << 31) - 256);   // GemmArgs::M is an int
    ARG_CHECK(colsum_pieces((int64_t)B * v.f.L) <= 65535);       // launch_colsum: the pieces are the grid's y
    for (int l = 0; l < cfg->layers; ++l) {
        const mpreid_vit_layer_t &t = wt->layers[l];
        ARG_CHECK(t.in_proj_t && t.out_proj_t && (l < n_moe || (t.fc_t && t.proj_t)));   // an MoE block has no dense MLP
        ARG_CHECK((((uintptr_t)t.in_proj_t | (uintptr_t)t.out_proj_t | (uintptr_t)t.fc_t | (uintptr_t)t.proj_t) & 15) == 0);
        if (grads) {
            const mpreid_vit_layer_grads &g = grads->layers[l];
            ARG_CHECK(l >= n_moe || !(g.fc_w || g.fc_b || g.proj_w || g.proj_b));
            ARG_CHECK((((uintptr_t)g.in_proj_w | (uintptr_t)g.in_proj_b | (uintptr_t)g.out_proj_w | (uintptr_t)g.out_proj_b |
                        (uintptr_t)g.fc_w | (uintptr_t)g.fc_b | (uintptr_t)g.proj_w | (uintptr_t)g.proj_b | (uintptr_t)g.ln1_g |
                        (uintptr_t)g.ln1_b | (uintptr_t)g.ln2_g | (uintptr_t)g.ln2_b) & 3) == 0);
        }
    }
    if (grads)
        ARG_CHECK((((uintptr_t)grads->conv_w | (uintptr_t)grads->class_emb | (uintptr_t)grads->pos_emb | (uintptr_t)grads->ln_pre_g |
                    (uintptr_t)grads->ln_pre_b | (uintptr_t)grads->ln_post_g | (uintptr_t)grads->ln_post_b |
                    (uintptr_t)grads->proj | (uintptr_t)grads->cv_emb) & 3) == 0);
    if (!ws || ws_bytes < v.total) {
        mpreid_set_error("vit backward workspace too small: %zu < %zu", ws_bytes, v.total);
        return MPREID_ERR_WORKSPACE;
    }
    ARG_CHECK(((uintptr_t)ws & 255) == 0);
    char *base = (char *)ws;
    auto f32 = [&](size_t off) { return (float *)(base + off); };
    BlockGrad c{};   // u is the sweep's use of the hbuf region: the same 16 W bytes per row
    c.s = {cfg->width, cfg->heads, B, v.f.L, false}; c.Mpad = v.f.Mpad; c.Mp4 = v.Mp4; c.stream = (hipStream_t)stream_;
    c.x = f32(v.f.x); c.a = (_Float16 *)(base + v.f.a); c.qkv = f32(v.f.qkv); c.u = f32(v.f.hbuf);
    c.dx = f32(v.r.dx); c.dh = f32(v.r.dh); c.t = f32(v.r.t); c.dqkv = f32(v.r.dqkv);
    c.aot = f32(v.aot); c.at = f32(v.at); c.bt = f32(v.bt); c.stats = base + v.stats; c.red = base + v.red;
    if ((rc = vit_backward_forward(c, cfg, w, moe, in, cv_emb, v, base))) return rc;
    if ((rc = vit_backward_head(c, w, grads, d_f, d_f_proj, cfg->out_dim, v.Bp4, f32(v.small)))) return rc;
    // an MoE tower's f_last is the CLS row of the LAST block's OUTPUT (model/clip/model.py:448-454): its seed joins dx in
    // front of the sweep
    if (moe && d_f_last && (rc = seed_f_last(c, d_f_last))) return rc;
    if ((rc = vit_backward_layers(c, cfg->layers, w, wt, grads, moe, moe_t, aux_coef, d_gate_w, l_aux_out, d_f_last, v, base)))
        return rc;
    return vit_backward_embed(c, w, grads, d_tokens, v, base);
}

}   // namespace

extern "C" int mpreid_vit_backward(const mpreid_vit_cfg *cfg, const mpreid_vit_weights *w, const mpreid_vit_weights_t *wt,
                                   const mpreid_image_in *img, int B, const float *cv_emb, const float *d_f_last,
                                   const float *d_f, const float *d_f_proj, const mpreid_vit_grads *grads, float *d_tokens,
                                   void *ws, size_t ws_bytes, mpreid_stream_t stream_) {
    return vit_backward_impl(cfg, w, wt, nullptr, nullptr, 0.f, nullptr, nullptr, img, B, cv_emb, d_f_last, d_f, d_f_proj, grads,
                             d_tokens, ws, ws_bytes, stream_);
}

extern "C" size_t mpreid_vit_backward_moe_workspace_bytes(const mpreid_vit_cfg *cfg, const mpreid_vit_moe *moe, int batch) {
    if (!cfg || !moe || batch <= 0 || vit_backward_check_cfg(cfg) || moe->moe_layers < 1) return 0;
    // (a query carries no pointers: only the shape checks of the call count)
    if (vit_check_moe_call(cfg, moe, batch) == MPREID_ERR_UNSUPPORTED) return 0;
    return vit_grad_layout(cfg, batch, moe).total;
}

extern "C" int mpreid_vit_backward_moe(const mpreid_vit_cfg *cfg, const mpreid_vit_weights *w, const mpreid_vit_weights_t *wt,
                                       const mpreid_vit_moe *moe, const mpreid_vit_moe_t *moe_t, const mpreid_image_in *img, int B,
                                       const float *cv_emb, const float *d_f_last, const float *d_f, const float *d_f_proj,
                                       float aux_coef, const mpreid_vit_grads *grads, float *d_gate_w, float *d_tokens,
                                       float *l_aux_out, void *ws, size_t ws_bytes, mpreid_stream_t stream_) {
    ARG_CHECK(moe != nullptr);
    return vit_backward_impl(cfg, w, wt, moe, moe_t, aux_coef, d_gate_w, l_aux_out, img, B, cv_emb, d_f_last, d_f, d_f_proj, grads,
                             d_tokens, ws, ws_bytes, stream_);
}
