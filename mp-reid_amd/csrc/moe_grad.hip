// moe_grad.hip — the gradient through one routed MLP of the MoE image tower and the gradient of its router, gfx950.
// Forward: csrc/moe.hip.  The experts' matrices are frozen in stage 2 (solver/make_optimizer_prompt.py: every name that
// contains "expert"), so what is computed here is the gradient THROUGH the experts and the gradient OF the routing weights:
//
//   per slot s = (row r, expert e = sel[r][k]):   u_s = c_fc_e(h_r)   t_s = QuickGELU(u_s)   y_s = c_proj_e(t_s) + b_proj_e
//   d_w[r][k] = <dy_r, y_s>                       dt_s = (w[r][k] dy_r) . Wproj_e           du_s = dt_s * QuickGELU'(u_s)
//   d_a[r]    = sum over the row's experts, ASCENDING e, of du_s . Wfc_e
//
//   recompute  the forward's own grouped GEMMs (moe_experts_launch): FC1 once more through the fp32 epilogue for u, then FC1 /
//              FC2 as in the forward for y.
//   GEMMs      one grouped exact-fp32 kernel, two epilogues, driven by the tile table and the device-side tile count the
//              dispatch left in the workspace.  v_mfma_f32_32x32x2_f32: per output element one k-ascending fp32 fmaf chain
//              from 0 (cdna_hip_programming.md 3, "FP32-input MFMA"), so the bits depend on no tiling and equal those of
//              mpreid_gemm_f32_linear on the same operands.  Tile and staging are gemm_f32_exact_kernel's (distance.hip):
//              128 x 128 per 256 threads, k tile 16, LDS [k][m] double-buffered, the next k tile's global loads in flight under
//              the MFMAs.  The A rows carry the slot -> row gather and the slot's routing weight; a padding slot stages zeros
//              and reads nothing.
//   d_w        one wave per row: lane-strided fmaf chains over the W features, the fixed butterfly, one rounded add when the
//              caller accumulates over MoE blocks.
//   combine    the ascending-e sum of moe_combine_kernel, without weights (they are inside du already).
//   router     one wave per row, 64 rows per wave: softmax as the forward's, c = sum_k w d_w, d_logits[sel_k] = w_k (d_w_k - c),
//              the load-balancing term p_j (g_j - sum_e p_e g_e); sum_r p[r][e] in pieces of 256 rows, pieces ascending.
// No atomics anywhere: every sum has one order.
#include "moe.h"

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int MOE_CNT_ROWS = 1024;   // rows per workgroup of the expert count
constexpr int MOE_RB_ROWS = 256;     // rows per workgroup of the router gradient: 4 waves x 64 rows, one piece of sum_r p

size_t moe_route_grad_bytes(int64_t rows, int E) {
    const size_t nblk = (size_t)((rows + MOE_CNT_ROWS - 1) / MOE_CNT_ROWS), npieces = (size_t)((rows + MOE_RB_ROWS - 1) / MOE_RB_ROWS);
    return align_up(nblk * E * 4, 256) + 256 + align_up(npieces * 64 * 4, 256);
}

MoeGradLayout moe_grad_layout(int64_t rows, int W, int E, int K) {
    MoeGradLayout g{};
    g.fwd = moe_layout(rows, W, E, K);
    g.npieces = (int)((rows + MOE_RB_ROWS - 1) / MOE_RB_ROWS);
    const size_t nblk = (size_t)((rows + MOE_CNT_ROWS - 1) / MOE_CNT_ROWS);
    size_t off = g.fwd.total;
    auto take = [&](size_t bytes) {
        size_t o = off;
        off += align_up(bytes, 256);
        return o;
    };
    g.u = take((size_t)g.fwd.slots_max * 4 * W * 4);
    g.slot_w = take((size_t)g.fwd.slots_max * 4);
    g.cnt_blk = take(nblk * E * 4);
    g.cnt = take(64 * 4);
    g.piece_p = take((size_t)g.npieces * 64 * 4);
    g.total = off;
    return g;
}

// ---------------------------------------------------------------------------------------------
// grouped exact-fp32 GEMM:  out[slot][n] = epi(sum_k s(slot) * A[row(slot)][k] * Wt[e][n][k]),  e = the expert of the slot's tile
// ---------------------------------------------------------------------------------------------
constexpr int GG_BK = 16, GG_LD = 132;

struct MoeGradGemmArgs {
    const float *A;          // fp32 [.][K]
    const int *gather;       // slot -> row of A (negative: a padding slot, staged as zeros); nullptr: row == slot
    const float *row_scale;  // [slots], read for live slots only; nullptr: 1
    const float *Wt;         // fp32 [E][N][K]
    const int2 *tile_tab;    // tile -> (expert, first slot)
    const int *ntiles;       // device-side tile count
    const float *u;          // SLOPE: fp32 [slots][N], the pre-activation; may be `out` itself (same element, same thread)
    float *out;              // fp32 [slots][N]
    int N, K, tiles_n, tiles_max;
};

__device__ __forceinline__ float quickgelu_slope(float t) {   // the expression of quickgelu_backward_kernel (text_grad.hip)
    const float sg = __fdiv_rn(1.0f, 1.0f + expf(-1.702f * t));
    return fmaf(1.702f * t * sg, 1.0f - sg, sg);
}

// N % 128 == 0, K % 16 == 0 (width % 128 == 0) and every tile's 128 slots lie inside the padded segment of its expert, so
// there is no edge in any dimension: slot0 + 127 < tiles_max * 128 = the row count of every per-slot buffer.
template <bool SLOPE>
__global__ __launch_bounds__(256) void moe_grad_gemm_kernel(MoeGradGemmArgs g) {
    __shared__ float Sm[2][2][GG_BK][GG_LD];
    float (&As)[2][GG_BK][GG_LD] = Sm[0];
    float (&Bs)[2][GG_BK][GG_LD] = Sm[1];
    int tm, tn;
    tile_coords(xcd_remap(blockIdx.x, gridDim.x), g.tiles_max, g.tiles_n, 8, tm, tn);
    if (tm >= *g.ntiles) return;   // uniform: the whole workgroup leaves before any barrier
    const int2 te = g.tile_tab[tm];
    const int ex = __builtin_amdgcn_readfirstlane(te.x), slot0 = __builtin_amdgcn_readfirstlane(te.y);
    const int n0 = tn * 128;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int li = lane & 31, lh = lane >> 5;
    const int K = g.K, N = g.N;

    // staging map of gemm_f32_exact_kernel: thread -> (row r0 + 64 r, float4 chunk kc) of a 128 x 16 k tile, per operand
    const int r0 = tid >> 2, kc = tid & 3;
    const float *arow[2], *brow[2];
    float asc[2];
    bool alive[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int slot = slot0 + r0 + 64 * r;
        const int ar = g.gather ? g.gather[slot] : slot;
        alive[r] = ar >= 0;
        asc[r] = (alive[r] && g.row_scale) ? g.row_scale[slot] : 1.0f;
        arow[r] = g.A + (int64_t)(alive[r] ? ar : 0) * K + kc * 4;
        brow[r] = g.Wt + ((int64_t)ex * N + n0 + r0 + 64 * r) * K + kc * 4;
    }
    float4 ra[2], rb[2];
    auto gload = [&](int kt) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
            if (alive[r]) {
                a = *reinterpret_cast<const float4 *>(arow[r] + kt * GG_BK);
                a.x = __fmul_rn(a.x, asc[r]);
                a.y = __fmul_rn(a.y, asc[r]);
                a.z = __fmul_rn(a.z, asc[r]);
                a.w = __fmul_rn(a.w, asc[r]);
            }
            ra[r] = a;
            rb[r] = *reinterpret_cast<const float4 *>(brow[r] + kt * GG_BK);
        }
    };
    auto sstore = [&](int buf) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int row = r0 + 64 * r;
            As[buf][kc * 4 + 0][row] = ra[r].x;
            As[buf][kc * 4 + 1][row] = ra[r].y;
            As[buf][kc * 4 + 2][row] = ra[r].z;
            As[buf][kc * 4 + 3][row] = ra[r].w;
            Bs[buf][kc * 4 + 0][row] = rb[r].x;
            Bs[buf][kc * 4 + 1][row] = rb[r].y;
            Bs[buf][kc * 4 + 2][row] = rb[r].z;
            Bs[buf][kc * 4 + 3][row] = rb[r].w;
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    const int nkt = K / GG_BK;
    gload(0);
    sstore(0);
    __syncthreads();
    for (int kt = 0; kt < nkt; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < nkt) gload(kt + 1);
        // lane l holds A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31]; k ascends across the MFMAs, and the operands of
        // the next k pair are read before the MFMAs of this one are issued (as in gemm_f32_exact_kernel)
        float a0 = As[buf][lh][wm * 64 + li], a1 = As[buf][lh][wm * 64 + 32 + li];
        float b0 = Bs[buf][lh][wn * 64 + li], b1 = Bs[buf][lh][wn * 64 + 32 + li];
#pragma unroll
        for (int kp = 0; kp < GG_BK / 2; ++kp) {
            float a0n = 0.f, a1n = 0.f, b0n = 0.f, b1n = 0.f;
            if (kp + 1 < GG_BK / 2) {
                a0n = As[buf][2 * kp + 2 + lh][wm * 64 + li];
                a1n = As[buf][2 * kp + 2 + lh][wm * 64 + 32 + li];
                b0n = Bs[buf][2 * kp + 2 + lh][wn * 64 + li];
                b1n = Bs[buf][2 * kp + 2 + lh][wn * 64 + 32 + li];
            }
            __builtin_amdgcn_sched_barrier(0);
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            a0 = a0n; a1 = a1n; b0 = b0n; b1 = b1n;
        }
        if (kt + 1 < nkt) sstore(buf ^ 1);
        __syncthreads();
    }

    // epilogue.  C/D map of the 32x32 MFMA: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int col = n0 + wn * 64 + j * 32 + li;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = slot0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                const int64_t idx = (int64_t)row * N + col;
                float v = acc[i][j][r];
                if constexpr (SLOPE) v = __fmul_rn(v, quickgelu_slope(g.u[idx]));
                g.out[idx] = v;
            }
        }
    }
}

template <bool SLOPE>
static int moe_grad_gemm_launch(const MoeGradGemmArgs &g, int64_t rows, hipStream_t stream) {
    void *ptok = mpreid_prof_begin(stream);
    hipLaunchKernelGGL(moe_grad_gemm_kernel<SLOPE>, dim3((unsigned)((int64_t)g.tiles_max * g.tiles_n)), dim3(256), 0, stream, g);
    mpreid_prof_end(ptok, stream, SLOPE ? MPREID_PROF_MOE_GRAD_DT : MPREID_PROF_MOE_GRAD_DH, rows, g.N, g.K, 0.0);
    LAUNCH_CHECK();
    return MPREID_OK;
}

// ---------------------------------------------------------------------------------------------
// slot <-> row kernels
// ---------------------------------------------------------------------------------------------
// slot_w[slot] = the routing weight of the (row, expert) the slot holds; padding slots are not written (and never read)
__global__ __launch_bounds__(256) void moe_slot_w_kernel(const int *__restrict__ tok_slot, const float *__restrict__ tok_w, int64_t n,
                                                         int64_t slots_max, float *__restrict__ slot_w) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int s = tok_slot[i];
    if (s >= 0 && s < slots_max) slot_w[s] = tok_w[i];
}

// One wave per row.  d_w[row][k] belongs to sel[row][k]; the row's slots are stored by ascending expert, so the slot of expert e
// is entry (number of the row's distinct valid experts below e).  An out-of-range entry gets 0; of a repeated expert the LAST
// entry owns the slot (the one whose weight the forward used) and the earlier ones get 0.
__global__ __launch_bounds__(256) void moe_dw_kernel(const float *__restrict__ dy, const float *__restrict__ y,
                                                     const int32_t *__restrict__ sel, const int *__restrict__ tok_slot, int64_t rows,
                                                     int W, int E, int K, int64_t slots_max, int accumulate, float *__restrict__ d_w) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    unsigned long long mask = 0ull;
    for (int k = 0; k < K; ++k) {
        const int s = sel[row * K + k];
        if ((unsigned)s < (unsigned)E) mask |= 1ull << s;
    }
    const float *dr = dy + row * (int64_t)W;
    for (int k = 0; k < K; ++k) {
        const int s = sel[row * K + k];
        bool ok = (unsigned)s < (unsigned)E;
        for (int k2 = k + 1; k2 < K; ++k2) ok = ok && sel[row * K + k2] != s;
        float v = 0.f;
        if (ok) {
            const int j = __popcll(mask & ((1ull << s) - 1ull));
            const int slot = tok_slot[row * K + j];
            if (slot >= 0 && slot < slots_max) {
                const float *yr = y + (int64_t)slot * W;
                float acc = 0.f;
                for (int c = lane * 4; c < W; c += 256) {
                    const float4 a = *reinterpret_cast<const float4 *>(dr + c);
                    const float4 b = *reinterpret_cast<const float4 *>(yr + c);
                    acc = fmaf(a.x, b.x, acc);
                    acc = fmaf(a.y, b.y, acc);
                    acc = fmaf(a.z, b.z, acc);
                    acc = fmaf(a.w, b.w, acc);
                }
                v = wave_bfly_add(acc);
            }
        }
        if (lane == 0) d_w[row * K + k] = accumulate ? __fadd_rn(d_w[row * K + k], v) : v;
    }
}

// d_a[row] = sum over the row's slots (ascending expert) of g[slot]; written, not added
__global__ __launch_bounds__(256) void moe_grad_combine_kernel(const float *__restrict__ g, const int *__restrict__ tok_slot,
                                                               int64_t rows, int W, int K, int64_t slots_max,
                                                               float *__restrict__ d_a) {
    const int w4 = W >> 2;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= rows * w4) return;
    const int64_t row = idx / w4;
    const int c = (int)(idx - row * w4) * 4;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int j = 0; j < K; ++j) {
        const int slot = tok_slot[row * K + j];
        if (slot < 0 || slot >= slots_max) continue;
        const float4 t = *reinterpret_cast<const float4 *>(g + (int64_t)slot * W + c);
        acc.x = __fadd_rn(acc.x, t.x);
        acc.y = __fadd_rn(acc.y, t.y);
        acc.z = __fadd_rn(acc.z, t.z);
        acc.w = __fadd_rn(acc.w, t.w);
    }
    *reinterpret_cast<float4 *>(d_a + row * W + c) = acc;
}

int moe_mlp_backward_launch(const _Float16 *a_pairs, const int32_t *sel, const MoeGradLayout &m, const mpreid_moe_layer *ly,
                            const mpreid_moe_layer_t *lt, const float *dy, float *d_a, float *d_w, bool accumulate_d_w, void *ws,
                            hipStream_t stream) {
    char *base = (char *)ws;
    const MoeLayout &f = m.fwd;
    const int W = f.W, K = f.K;
    float *u = (float *)(base + m.u);
    float *y = (float *)(base + f.y);
    float *slot_w = (float *)(base + m.slot_w);
    const int *tok_slot = (const int *)(base + f.tok_slot);
    int rc = moe_experts_launch(a_pairs, f, ly, ws, u, stream);   // u, and y[slot] with the forward's bits
    if (rc) return rc;
    if (d_w) {
        void *ptok = mpreid_prof_begin(stream);
        hipLaunchKernelGGL(moe_dw_kernel, dim3((unsigned)((f.rows + 3) / 4)), dim3(256), 0, stream, dy, (const float *)y, sel, tok_slot,
                           f.rows, W, f.E, K, f.slots_max, accumulate_d_w ? 1 : 0, d_w);
        mpreid_prof_end(ptok, stream, MPREID_PROF_MOE_GRAD_DW, f.rows, f.E, K, 0.0);
        LAUNCH_CHECK();
    }
    if (!d_a) return MPREID_OK;
    const int64_t nk = f.rows * K;
    hipLaunchKernelGGL(moe_slot_w_kernel, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, stream, tok_slot,
                       (const float *)(base + f.tok_w), nk, f.slots_max, slot_w);
    LAUNCH_CHECK();
    MoeGradGemmArgs g{};
    g.tile_tab = (const int2 *)(base + f.tile_tab);
    g.ntiles = (const int *)(base + f.meta);
    g.tiles_max = f.tiles_max;
    // du[slot] = ((w dy[row(slot)]) . Wproj_e) * QuickGELU'(u[slot]), in place over u
    g.A = dy;
    g.gather = (const int *)(base + f.slot_row);
    g.row_scale = slot_w;
    g.Wt = lt->proj_t;
    g.N = 4 * W;
    g.K = W;
    g.tiles_n = g.N / 128;
    g.u = u;
    g.out = u;
    if ((rc = moe_grad_gemm_launch<true>(g, f.rows, stream))) return rc;
    // g[slot] = du[slot] . Wfc_e, over y (d_w has been taken from it)
    g.A = u;
    g.gather = nullptr;
    g.row_scale = nullptr;
    g.Wt = lt->fc_t;
    g.N = W;
    g.K = 4 * W;
    g.tiles_n = g.N / 128;
    g.u = nullptr;
    g.out = y;
    if ((rc = moe_grad_gemm_launch<false>(g, f.rows, stream))) return rc;
    const int64_t n4 = f.rows * (W / 4);
    void *ptok = mpreid_prof_begin(stream);
    hipLaunchKernelGGL(moe_grad_combine_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, stream, (const float *)y, tok_slot,
                       f.rows, W, K, f.slots_max, d_a);
    mpreid_prof_end(ptok, stream, MPREID_PROF_MOE_GRAD_COMBINE, f.rows, f.E, K, 0.0);
    LAUNCH_CHECK();
    return MPREID_OK;
}

// ---------------------------------------------------------------------------------------------
// router gradient
// ---------------------------------------------------------------------------------------------
// The unit seam's own count (the tower reads the dispatch's, moe.h MOE_META_COUNTS).
// cnt_blk[blk][e] = rows of this workgroup's 1024 that chose e (distinct valid entries of sel, as the dispatch counts them)
__global__ __launch_bounds__(256) void moe_count_kernel(const int32_t *__restrict__ sel, int64_t rows, int E, int K,
                                                        int *__restrict__ cnt_blk) {
    __shared__ int wcnt[16][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t row0 = (int64_t)blockIdx.x * MOE_CNT_ROWS;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int c = it * 4 + wave;
        const int64_t row = row0 + c * 64 + lane;
        unsigned long long mask = 0ull;
        if (row < rows)
            for (int k = 0; k < K; ++k) {
                const int s = sel[row * K + k];
                if ((unsigned)s < (unsigned)E) mask |= 1ull << s;
            }
        for (int e = 0; e < E; ++e) {
            const unsigned long long b = __ballot((mask >> e) & 1ull);
            if (lane == 0) wcnt[c][e] = __popcll(b);
        }
    }
    __syncthreads();
    if (tid < E) {
        int s = 0;
#pragma unroll
        for (int c = 0; c < 16; ++c) s += wcnt[c][tid];
        cnt_blk[(int64_t)blockIdx.x * E + tid] = s;
    }
}

__global__ __launch_bounds__(64) void moe_count_sum_kernel(const int *__restrict__ cnt_blk, int nblk, int E, int *__restrict__ cnt) {
    const int e = threadIdx.x;
    int s = 0;
    if (e < E)
        for (int b = 0; b < nblk; ++b) s += cnt_blk[(int64_t)b * E + e];
    cnt[e] = s;
}

// One wave per row, 64 consecutive rows per wave, lane e = expert e.  piece_p[workgroup][e] = sum of p[row][e] over the
// workgroup's 256 rows: per wave rows ascending, then the four waves in order.
__global__ __launch_bounds__(256) void moe_route_backward_kernel(const float *__restrict__ logits, const int32_t *__restrict__ sel,
                                                                 const float *__restrict__ w, const float *__restrict__ d_w,
                                                                 const int *__restrict__ cnt, int64_t rows, int E, int K, float coef,
                                                                 float *__restrict__ d_logits, float *__restrict__ piece_p) {
    __shared__ float part[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // g_e = coef * E * f_e / rows, f_e = count_e / rows.  p_j (g_j - sum_e p_e g_e) does not change when a constant is taken
    // off every g_e (sum_e p_e = 1), so the mean goes first, in integers: E count_e - sum_e count_e is exact, and what is left
    // of g no longer cancels against its own average (counts are close to each other when the router is balanced)
    const float frows = (float)rows;
    const int ce = lane < E ? cnt[lane] : 0;
    int ctot = ce;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) ctot += __shfl_xor(ctot, off, 64);
    const float ge = lane < E ? __fdiv_rn(__fdiv_rn(__fmul_rn(coef, (float)(E * ce - ctot)), frows), frows) : 0.f;
    float psum = 0.f;
    const int64_t row0 = (int64_t)blockIdx.x * MOE_RB_ROWS + wave * 64;
    for (int i = 0; i < 64; ++i) {
        const int64_t row = row0 + i;
        if (row >= rows) break;
        const float logit = lane < E ? logits[row * E + lane] : -INFINITY;
        float mx = logit;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
        const float ex = lane < E ? expf(logit - mx) : 0.f;
        const float den = wave_bfly_add(ex);
        const float p = ex / den;
        psum = __fadd_rn(psum, p);
        if (!d_logits) continue;
        float d = 0.f;
        if (d_w) {
            float c = 0.f;
            for (int k = 0; k < K; ++k) c = fmaf(w[row * K + k], d_w[row * K + k], c);
            for (int k = 0; k < K; ++k)   // an out-of-range entry matches no lane; of a repeated expert the last entry stays
                if (lane == sel[row * K + k]) d = __fmul_rn(w[row * K + k], __fsub_rn(d_w[row * K + k], c));
        }
        if (coef != 0.f) {
            const float pg = wave_bfly_add(__fmul_rn(p, ge));
            d = __fadd_rn(d, __fmul_rn(p, __fsub_rn(ge, pg)));
        }
        if (lane < E) d_logits[row * E + lane] = d;
    }
    part[wave][lane] = psum;
    __syncthreads();
    if (wave == 0) piece_p[(int64_t)blockIdx.x * 64 + lane] = ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
}

// l_aux = E * sum_e f_e P_e: P_e = (sum of the pieces, ascending) / rows, then the experts ascending
__global__ __launch_bounds__(64) void moe_laux_kernel(const float *__restrict__ piece_p, int npieces, const int *__restrict__ cnt,
                                                      int64_t rows, int E, float *__restrict__ l_aux) {
    const int lane = threadIdx.x;
    float s = 0.f;
    for (int i = 0; i < npieces; ++i) s = __fadd_rn(s, piece_p[(int64_t)i * 64 + lane]);
    const float frows = (float)rows;
    const float term = lane < E ? __fmul_rn(__fdiv_rn((float)cnt[lane], frows), __fdiv_rn(s, frows)) : 0.f;
    float tot = 0.f;
    for (int e = 0; e < E; ++e) tot = __fadd_rn(tot, __shfl(term, e, 64));
    if (lane == 0) *l_aux = __fmul_rn((float)E, tot);
}

int moe_route_backward_launch(const float *logits, const int32_t *sel, const float *w, const float *d_w, int64_t rows, int E, int K,
                              float aux_coef, float *d_logits, float *l_aux, const int *dispatch_cnt, int *cnt_blk, int *cnt,
                              float *piece_p, hipStream_t stream) {
    const int nblk = (int)((rows + MOE_CNT_ROWS - 1) / MOE_CNT_ROWS), npieces = (int)((rows + MOE_RB_ROWS - 1) / MOE_RB_ROWS);
    void *ptok = mpreid_prof_begin(stream);
    const int *counts = dispatch_cnt;
    if (!counts) {   // the unit seam: no dispatch has run for this sel
        hipLaunchKernelGGL(moe_count_kernel, dim3((unsigned)nblk), dim3(256), 0, stream, sel, rows, E, K, cnt_blk);
        hipLaunchKernelGGL(moe_count_sum_kernel, dim3(1), dim3(64), 0, stream, (const int *)cnt_blk, nblk, E, cnt);
        counts = cnt;
    }
    hipLaunchKernelGGL(moe_route_backward_kernel, dim3((unsigned)npieces), dim3(256), 0, stream, logits, sel, w, d_w, counts, rows, E,
                       K, aux_coef, d_logits, piece_p);
    if (l_aux)
        hipLaunchKernelGGL(moe_laux_kernel, dim3(1), dim3(64), 0, stream, (const float *)piece_p, npieces, counts, rows, E, l_aux);
    mpreid_prof_end(ptok, stream, MPREID_PROF_MOE_GRAD_ROUTER, rows, E, K, 0.0);
    LAUNCH_CHECK();
    return MPREID_OK;
}

bool moe_coef_is_finite(float aux_coef) { return aux_coef == aux_coef && aux_coef - aux_coef == 0.f; }

int moe_route_backward_ws(const float *logits, const int32_t *sel, const float *w, const float *d_w, int64_t rows, int E, int K,
                          float aux_coef, float *d_logits, float *l_aux, const int *dispatch_cnt, void *ws, hipStream_t stream) {
    const size_t cb = align_up((size_t)((rows + MOE_CNT_ROWS - 1) / MOE_CNT_ROWS) * E * 4, 256);
    char *base = (char *)ws;
    return moe_route_backward_launch(logits, sel, w, d_w, rows, E, K, aux_coef, d_logits, l_aux, dispatch_cnt, (int *)base,
                                     (int *)(base + cb), (float *)(base + cb + 256), stream);
}

__global__ __launch_bounds__(256) void moe_gate_dh_kernel(const float *__restrict__ d_logits, const float *__restrict__ gate,
                                                          int64_t rows, int W, int E, float *__restrict__ t) {
    const int w4 = W >> 2;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= rows * w4) return;
    const int64_t row = idx / w4;
    const int c = (int)(idx - row * w4) * 4;
    float4 acc = *reinterpret_cast<const float4 *>(t + row * W + c);
    for (int e = 0; e < E; ++e) {
        const float d = d_logits[row * E + e];
        const float4 gw = *reinterpret_cast<const float4 *>(gate + (int64_t)e * W + c);
        acc.x = fmaf(d, gw.x, acc.x);
        acc.y = fmaf(d, gw.y, acc.y);
        acc.z = fmaf(d, gw.z, acc.z);
        acc.w = fmaf(d, gw.w, acc.w);
    }
    *reinterpret_cast<float4 *>(t + row * W + c) = acc;
}

int moe_gate_dh_launch(const float *d_logits, const float *gate, int64_t rows, int W, int E, float *t, hipStream_t stream) {
    const int64_t n4 = rows * (W / 4);
    hipLaunchKernelGGL(moe_gate_dh_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, stream, d_logits, gate, rows, W, E, t);
    LAUNCH_CHECK();
    return MPREID_OK;
}

// ---------------------------------------------------------------------------------------------
// C ABI: the unit seams
// ---------------------------------------------------------------------------------------------
extern "C" size_t mpreid_moe_grad_workspace_bytes(int64_t rows, int width, int E, int K) {
    if (rows <= 0 || moe_check_shape(rows, width, E, K)) return 0;
    return moe_grad_layout(rows, width, E, K).total;
}

extern "C" int mpreid_moe_mlp_backward(const void *a_pairs, int64_t rows, int width, const int32_t *sel, const float *w, int E, int K,
                                       const mpreid_moe_layer *ly, const mpreid_moe_layer_t *lt, const float *dy, float *d_a,
                                       float *d_w, int accumulate_d_w, const mpreid_moe_expert_grads *d_experts, void *ws,
                                       size_t ws_bytes, mpreid_stream_t stream) {
    int rc = moe_check_shape(rows, width, E, K);
    if (rc) return rc;
    if (d_experts && (d_experts->fc_w || d_experts->fc_b || d_experts->proj_w || d_experts->proj_b)) {
        mpreid_set_error("MoE backward: the expert matrices' own gradients are not implemented (d_experts must be NULL or all "
                         "NULL); missing: the grouped weight-gradient GEMMs du^T h and dy^T t per expert segment");
        return MPREID_ERR_UNSUPPORTED;
    }
    ARG_CHECK(a_pairs && sel && w && dy && rows > 0 && (d_a || d_w));
    if ((rc = moe_check_layer(ly))) return rc;
    ARG_CHECK(lt && lt->fc_t && lt->proj_t && ((uintptr_t)lt->fc_t & 15) == 0 && ((uintptr_t)lt->proj_t & 15) == 0);
    ARG_CHECK(((uintptr_t)a_pairs & 15) == 0 && ((uintptr_t)dy & 15) == 0 && ((uintptr_t)d_a & 15) == 0 &&
              ((uintptr_t)sel & 3) == 0 && ((uintptr_t)w & 3) == 0 && ((uintptr_t)d_w & 3) == 0);
    ARG_CHECK(((uintptr_t)ws & 255) == 0);
    const MoeGradLayout m = moe_grad_layout(rows, width, E, K);
    if (!ws || ws_bytes < m.total) {
        mpreid_set_error("MoE gradient workspace too small: %zu < %zu", ws_bytes, m.total);
        return MPREID_ERR_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    if ((rc = moe_dispatch_launch(sel, w, m.fwd, ws, s))) return rc;
    return moe_mlp_backward_launch(reinterpret_cast<const _Float16 *>(a_pairs), sel, m, ly, lt, dy, d_a, d_w, accumulate_d_w != 0, ws, s);
}

extern "C" size_t mpreid_moe_route_backward_workspace_bytes(int64_t rows, int E) {
    if (rows <= 0 || moe_check_shape(rows, 128, E, 1)) return 0;
    return moe_route_grad_bytes(rows, E);
}

extern "C" int mpreid_moe_route_backward(const float *logits, int64_t rows, int E, int K, const int32_t *sel, const float *w,
                                         const float *d_w, float aux_coef, float *d_logits, float *l_aux, void *ws, size_t ws_bytes,
                                         mpreid_stream_t stream) {
    int rc = moe_check_shape(rows, 128, E, K);   // no width here: any valid one
    if (rc) return rc;
    ARG_CHECK(logits && sel && w && rows > 0 && (d_logits || l_aux));
    ARG_CHECK(((uintptr_t)logits & 3) == 0 && ((uintptr_t)sel & 3) == 0 && ((uintptr_t)w & 3) == 0 && ((uintptr_t)d_w & 3) == 0 &&
              ((uintptr_t)d_logits & 3) == 0 && ((uintptr_t)l_aux & 3) == 0);
    ARG_CHECK(moe_coef_is_finite(aux_coef));
    ARG_CHECK(((uintptr_t)ws & 255) == 0);
    const size_t need = moe_route_grad_bytes(rows, E);
    if (!ws || ws_bytes < need) {
        mpreid_set_error("MoE router gradient workspace too small: %zu < %zu", ws_bytes, need);
        return MPREID_ERR_WORKSPACE;
    }
    return moe_route_backward_ws(logits, sel, w, d_w, rows, E, K, aux_coef, d_logits, l_aux, nullptr, ws, (hipStream_t)stream);
}
