// moe.hip — the mixture-of-experts MLP of the image tower (model/clip/model.py:163-258, 283-330), gfx950.
//
//   router     one wave per token row: LayerNorm (the arithmetic of vit.hip's layernorm_kernel), E fp32 dot products in a
//              fixed order, softmax, top-k (ties: lower expert first), renormalisation.  No fp16 anywhere: a discrete
//              decision must not ride on operand rounding.
//   dispatch   sel -> per-expert counts -> exclusive scan -> slot table, all on the device.  Expert e owns a contiguous
//              slot segment, padded to the GEMM's 128-row tile, that holds its tokens in ASCENDING row order (ranks come
//              from ballots and prefix sums, never from the arrival order of atomics).  A tile table maps a workgroup's
//              tile to (expert, first slot); the grid is sized by the host-computable worst case and workgroups past the
//              device-side tile count exit.
//   GEMMs      one grouped split-precision kernel, two epilogues: 128 x 128 tile, 4 waves, fp16 pair operands, per 32-wide
//              k block hi.hi' + lo.hi' + hi.lo' into one fp32 accumulator (the order of gemm_f16.hip's split mode).  A k block
//              of an operand is one LDS row [hi(32) | lo(32)] = 128 bytes, filled by LDS-DMA whose per-lane SOURCE address
//              carries the A-row gather (slot -> token row) and the bank swizzle (16-byte chunk ^= row & 7, applied again
//              on the ds_read_b128 address: cdna_hip_programming.md 5.4 rule 21).  Two 32 KB stages: the DMA of k block
//              t + 1 is in flight under the 48 MFMAs of block t; 64 KB per workgroup, so two workgroups share a CU and
//              overlap each other's barriers.
//   combine    per token row acc = 0; for e in sel ascending: acc = fl(acc + fl(w_e * y[slot(token, e)])); x += acc.
//              One kernel, no atomics: the bits do not depend on the geometry.
#include "gemm_f16.h"
#include "moe.h"

typedef __attribute__((address_space(3))) void moe_lds_ptr_t;
typedef const __attribute__((address_space(1))) void moe_glb_ptr_t;

__device__ __forceinline__ void moe_dma16(const void *gsrc, unsigned char *lds_dst_wave_base) {
    // LDS destination = wave-uniform base + lane * 16; the global source is per lane
    __builtin_amdgcn_global_load_lds((moe_glb_ptr_t *)gsrc, (moe_lds_ptr_t *)lds_dst_wave_base, 16, 0, 0);
}

// ---------------------------------------------------------------------------------------------
// layout of the workspace
// ---------------------------------------------------------------------------------------------
constexpr int MOE_ROWS_PER_BLOCK = 1024;   // dispatch kernels: 16 sub-chunks of 64 rows (one wave each) per workgroup
constexpr int MOE_META_INTS = 256;         // [0] tile count, [64 .. 64 + E) first slot of expert e, [128 .. 128 + E) rows of expert e

MoeLayout moe_layout(int64_t rows, int W, int E, int K) {
    MoeLayout m{};
    m.rows = rows; m.W = W; m.E = E; m.K = K;
    m.tiles_max = (int)((rows * K + MOE_BM - 1) / MOE_BM) + E;   // sum_e ceil(c_e / 128) <= ceil(rows K / 128) + E
    m.slots_max = (int64_t)m.tiles_max * MOE_BM;
    m.nblk = (int)((rows + MOE_ROWS_PER_BLOCK - 1) / MOE_ROWS_PER_BLOCK);
    size_t off = 0;
    auto take = [&](size_t bytes) {
        size_t o = off;
        off += align_up(bytes, 256);
        return o;
    };
    m.meta = take(MOE_META_INTS * 4);
    m.tile_tab = take((size_t)m.tiles_max * 8);
    m.blk_cnt = take((size_t)m.nblk * E * 4);
    m.slot_row = take((size_t)m.slots_max * 4);
    m.tok_slot = take((size_t)rows * K * 4);
    m.tok_w = take((size_t)rows * K * 4);
    m.hidden = take((size_t)m.slots_max * 8 * W * 2);   // fp16 pairs [slots][hi(4W) | lo(4W)]
    m.y = take((size_t)m.slots_max * W * 4);
    m.total = off;
    return m;
}

int moe_check_shape(int64_t rows, int W, int E, int K) {
    if (E < 1 || E > MPREID_MOE_MAX_EXPERTS || K < 1 || K > MPREID_MOE_MAX_TOPK || K > E) {
        mpreid_set_error("MoE: need 1 <= top_k <= min(num_experts, %d) and num_experts <= %d (num_experts %d, top_k %d)",
                         MPREID_MOE_MAX_TOPK, MPREID_MOE_MAX_EXPERTS, E, K);
        return MPREID_ERR_UNSUPPORTED;
    }
    if (W <= 0 || W % 128 != 0 || W > 1024) {
        mpreid_set_error("MoE: width %d is not a multiple of 128 in 128 .. 1024", W);
        return MPREID_ERR_UNSUPPORTED;
    }
    // One workgroup scans the per-workgroup counts (moe_scan_kernel: a serial walk over ceil(rows / 1024) entries per expert,
    // microseconds at the 65 536 rows of an encoder call, ~0.1 ms at the limit); slot and tile indices are 32-bit.
    if (rows > MPREID_MOE_MAX_ROWS) {
        mpreid_set_error("MoE: %lld token rows in one call are more than MPREID_MOE_MAX_ROWS (%d)", (long long)rows,
                         MPREID_MOE_MAX_ROWS);
        return MPREID_ERR_UNSUPPORTED;
    }
    return MPREID_OK;
}

// ---------------------------------------------------------------------------------------------
// router
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long k) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)k, off, 64), hi = __shfl_xor((unsigned)(k >> 32), off, 64);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        k = o > k ? o : k;
    }
    return k;
}

// One wave per row, whatever the launch: a row's result depends on nothing but the row.
template <bool LN>
__global__ __launch_bounds__(256) void moe_router_kernel(const float *__restrict__ x, int64_t rows, int W,
                                                         const float *__restrict__ gamma, const float *__restrict__ beta,
                                                         const float *__restrict__ gate, int E, int K,
                                                         int32_t *__restrict__ sel, float *__restrict__ wout,
                                                         float *__restrict__ logits) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float *xr = x + row * (int64_t)W;
    float4 v[4];   // W <= 1024
    bool act[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        act[i] = (i * 256 + lane * 4) < W;
        v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (act[i]) v[i] = *reinterpret_cast<const float4 *>(xr + i * 256 + lane * 4);
    }
    if constexpr (LN) {   // the statistics and the affine step of layernorm_kernel, operation for operation
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
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
            v[i].x = (v[i].x - mean) * rstd * gm.x + bt.x;
            v[i].y = (v[i].y - mean) * rstd * gm.y + bt.y;
            v[i].z = (v[i].z - mean) * rstd * gm.z + bt.z;
            v[i].w = (v[i].w - mean) * rstd * gm.w + bt.w;
        }
    }
    // logits: per lane an fmaf chain over its columns in ascending order, then the fixed butterfly; lane e keeps logit e
    float logit = -INFINITY;
    for (int e = 0; e < E; ++e) {
        const float *gr = gate + (int64_t)e * W;
        float p = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (act[i]) {
                const float4 gw = *reinterpret_cast<const float4 *>(gr + i * 256 + lane * 4);
                p = fmaf(v[i].x, gw.x, p);
                p = fmaf(v[i].y, gw.y, p);
                p = fmaf(v[i].z, gw.z, p);
                p = fmaf(v[i].w, gw.w, p);
            }
        }
        p = wave_bfly_add(p);
        if (lane == e) logit = p;
    }
    if (logits && lane < E) logits[row * E + lane] = logit;
    // softmax over the E lanes
    float mx = logit;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
    const float ex = lane < E ? expf(logit - mx) : 0.f;
    const float den = wave_bfly_add(ex);
    const float p = ex / den;
    // top-k: K rounds of (largest p, lowest lane); lane k keeps round k
    bool taken = lane >= E;
    float psum = 0.f, myp = 0.f;
    int mysel = 0;
    for (int k = 0; k < K; ++k) {
        const unsigned long long key =
            taken ? 0ull : (((unsigned long long)__float_as_uint(p) << 32) | (unsigned)(64 - lane));
        const unsigned long long best = wave_max_u64(key);
        const int win = 64 - (int)(best & 0xffu);
        const float pk = __uint_as_float((unsigned)(best >> 32));
        if (lane == win) taken = true;
        if (lane == k) {
            mysel = win;
            myp = pk;
        }
        psum = psum + pk;
    }
    if (lane < K) {
        sel[row * K + lane] = mysel;
        wout[row * K + lane] = myp / psum;
    }
}

int moe_route_launch(const float *x, int64_t rows, int W, const float *ln_g, const float *ln_b, const float *gate, int E, int K,
                     int32_t *sel, float *w, float *logits, hipStream_t stream) {
    const dim3 grid((unsigned)((rows + 3) / 4));
    void *ptok = mpreid_prof_begin(stream);
    if (ln_g)
        hipLaunchKernelGGL(moe_router_kernel<true>, grid, dim3(256), 0, stream, x, rows, W, ln_g, ln_b, gate, E, K, sel, w, logits);
    else
        hipLaunchKernelGGL(moe_router_kernel<false>, grid, dim3(256), 0, stream, x, rows, W, ln_g, ln_b, gate, E, K, sel, w, logits);
    mpreid_prof_end(ptok, stream, MPREID_PROF_MOE_ROUTER, rows, E, K, 0.0);
    LAUNCH_CHECK();
    return MPREID_OK;
}

// ---------------------------------------------------------------------------------------------
// dispatch
// ---------------------------------------------------------------------------------------------
// the experts of a row as a 64-bit mask (values outside 0 .. E-1 are dropped: such a row simply gets fewer terms)
__device__ __forceinline__ unsigned long long moe_row_mask(const int32_t *__restrict__ sel, int64_t row, int64_t rows, int E, int K) {
    unsigned long long m = 0ull;
    if (row < rows)
        for (int k = 0; k < K; ++k) {
            const int s = sel[row * K + k];
            if ((unsigned)s < (unsigned)E) m |= 1ull << s;
        }
    return m;
}

// PLACE false: blk_cnt[blk][e] = rows of this workgroup's 1024 that chose e, and slot_row = -1 everywhere.
// PLACE true: the same counts again, then slot_row / tok_slot / tok_w from the scanned tables.
template <bool PLACE>
__global__ __launch_bounds__(256) void moe_dispatch_kernel(const int32_t *__restrict__ sel, const float *__restrict__ w,
                                                           int64_t rows, int E, int K, int *__restrict__ blk_cnt,
                                                           const int *__restrict__ meta, int *__restrict__ slot_row,
                                                           int64_t slots_max, int *__restrict__ tok_slot,
                                                           float *__restrict__ tok_w) {
    __shared__ int wcnt[16][64];   // [sub-chunk of 64 rows][expert]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t row0 = (int64_t)blockIdx.x * MOE_ROWS_PER_BLOCK;
    unsigned long long mask[4];
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int c = it * 4 + wave;
        mask[it] = moe_row_mask(sel, row0 + c * 64 + lane, rows, E, K);
        for (int e = 0; e < E; ++e) {
            const unsigned long long b = __ballot((mask[it] >> e) & 1ull);
            if (lane == 0) wcnt[c][e] = __popcll(b);
        }
    }
    __syncthreads();
    if constexpr (!PLACE) {
        if (tid < E) {
            int s = 0;
#pragma unroll
            for (int c = 0; c < 16; ++c) s += wcnt[c][tid];
            blk_cnt[(int64_t)blockIdx.x * E + tid] = s;
        }
        for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < slots_max; i += (int64_t)gridDim.x * 256) slot_row[i] = -1;
    } else {
        if (tid < E) {   // exclusive prefix over the sub-chunks, on top of the expert's segment start and this workgroup's base
            int run = meta[64 + tid] + blk_cnt[(int64_t)blockIdx.x * E + tid];
#pragma unroll
            for (int c = 0; c < 16; ++c) {
                const int n = wcnt[c][tid];
                wcnt[c][tid] = run;
                run += n;
            }
        }
        __syncthreads();
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int c = it * 4 + wave;
            const int64_t row = row0 + c * 64 + lane;
            int j = 0;
            for (int e = 0; e < E; ++e) {
                const bool has = (mask[it] >> e) & 1ull;
                const unsigned long long b = __ballot(has);
                if (has) {
                    const int slot = wcnt[c][e] + __popcll(b & ((1ull << lane) - 1ull));
                    slot_row[slot] = (int)row;
                    float wv = 0.f;
                    for (int k = 0; k < K; ++k)
                        if (sel[row * K + k] == e) wv = w[row * K + k];
                    tok_slot[row * K + j] = slot;
                    tok_w[row * K + j] = wv;
                    ++j;
                }
            }
            if (row < rows)
                for (; j < K; ++j) tok_slot[row * K + j] = -1;   // only with out-of-range or repeated entries in sel
        }
    }
}

// one workgroup: blk_cnt[b][e] -> exclusive scan over b; segment starts (padded to the row tile), tile table, tile count
__global__ __launch_bounds__(64) void moe_scan_kernel(int *__restrict__ blk_cnt, int nblk, int E, int *__restrict__ meta,
                                                      int2 *__restrict__ tile_tab) {
    __shared__ int cnt[64], seg[64], tbase[64];
    const int e = threadIdx.x;
    if (e < E) {
        int run = 0;
#pragma unroll 8
        for (int b = 0; b < nblk; ++b) {
            const int c = blk_cnt[(int64_t)b * E + e];
            blk_cnt[(int64_t)b * E + e] = run;
            run += c;
        }
        cnt[e] = run;
    }
    __syncthreads();
    if (e == 0) {
        int off = 0, t = 0;
        for (int i = 0; i < E; ++i) {
            seg[i] = off;
            tbase[i] = t;
            const int nt = (cnt[i] + MOE_BM - 1) / MOE_BM;
            off += nt * MOE_BM;
            t += nt;
        }
        meta[0] = t;
    }
    __syncthreads();
    if (e < E) {
        meta[64 + e] = seg[e];
        meta[MOE_META_COUNTS + e] = cnt[e];   // (read by the router's gradient: the shares f_e of the load-balancing loss)
        const int nt = (cnt[e] + MOE_BM - 1) / MOE_BM;
        for (int i = 0; i < nt; ++i) tile_tab[tbase[e] + i] = make_int2(e, seg[e] + i * MOE_BM);
    }
}

int moe_dispatch_launch(const int32_t *sel, const float *w, const MoeLayout &m, void *ws, hipStream_t stream) {
    char *base = (char *)ws;
    int *meta = (int *)(base + m.meta);
    int2 *tile_tab = (int2 *)(base + m.tile_tab);
    int *blk_cnt = (int *)(base + m.blk_cnt);
    int *slot_row = (int *)(base + m.slot_row);
    int *tok_slot = (int *)(base + m.tok_slot);
    float *tok_w = (float *)(base + m.tok_w);
    void *ptok = mpreid_prof_begin(stream);
    hipLaunchKernelGGL(moe_dispatch_kernel<false>, dim3((unsigned)m.nblk), dim3(256), 0, stream, sel, w, m.rows, m.E, m.K, blk_cnt,
                       (const int *)meta, slot_row, m.slots_max, tok_slot, tok_w);
    hipLaunchKernelGGL(moe_scan_kernel, dim3(1), dim3(64), 0, stream, blk_cnt, m.nblk, m.E, meta, tile_tab);
    hipLaunchKernelGGL(moe_dispatch_kernel<true>, dim3((unsigned)m.nblk), dim3(256), 0, stream, sel, w, m.rows, m.E, m.K, blk_cnt,
                       (const int *)meta, slot_row, m.slots_max, tok_slot, tok_w);
    mpreid_prof_end(ptok, stream, MPREID_PROF_MOE_DISPATCH, m.rows, m.E, m.K, 0.0);
    LAUNCH_CHECK();
    return MPREID_OK;
}

// ---------------------------------------------------------------------------------------------
// grouped split-precision GEMM:  out[slot][n] = epi(sum_k A[row(slot)][k] * W[e][n][k]),  e = the expert of the slot's tile
// ---------------------------------------------------------------------------------------------
constexpr int MG_BK = 32;                          // k block: 32 hi + 32 lo halfs = one 128-byte LDS row
constexpr int MG_TILE_BYTES = MOE_BM * 128;        // 16 KB per operand
constexpr int MG_STAGE_BYTES = 2 * MG_TILE_BYTES;  // A + B
constexpr int MG_LDS_BYTES = 2 * MG_STAGE_BYTES;   // two stages: 64 KB

struct MoeGemmArgs {
    const _Float16 *A;       // fp16 pairs [.][2 * kseg]
    const int *gather;       // slot -> row of A (negative: a padding slot, reads row 0); nullptr: row == slot
    const _Float16 *W;       // fp16 pairs [E][N][2 * kseg]
    const float *bias;       // [E][N]
    const float *scale;      // [E]: 2^-e of the expert's matrix
    const int2 *tile_tab;    // tile -> (expert, first slot)
    const int *ntiles;       // device-side tile count
    int N, kseg, tiles_n, tiles_max;
    void *out;               // MG_GELU_PAIR: fp16 [slots][2N]; MG_F32: fp32 [slots][N]
};
enum { MG_GELU_PAIR = 0, MG_F32 = 1 };

template <int EPI>
__global__ __launch_bounds__(256, 2) void moe_gemm_kernel(MoeGemmArgs g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int tm, tn;
    tile_coords(xcd_remap(blockIdx.x, gridDim.x), g.tiles_max, g.tiles_n, 8, tm, tn);
    if (tm >= *g.ntiles) return;   // uniform: the whole workgroup leaves before any barrier
    const int2 te = g.tile_tab[tm];
    const int ex = __builtin_amdgcn_readfirstlane(te.x), slot0 = __builtin_amdgcn_readfirstlane(te.y);
    const int n0 = tn * 128;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int K2 = 2 * g.kseg, N = g.N;
    const int nkb = g.kseg / MG_BK;

    // ---- staging: wave w moves rows [32w, 32w + 32) of both tiles, 8 rows per DMA instruction.  LDS slot (lane & 7) of row
    // srow receives logical chunk c = (lane & 7) ^ srow of the row [hi(32) | lo(32)]: chunks 0-3 come from the hi half of the
    // source row, 4-7 from its lo half, kseg halfs further on.
    const int srow = lane >> 3;
    const int lchunk = (lane & 7) ^ srow;
    const int64_t coff = (lchunk & 3) * 8 + (lchunk >> 2) * (int64_t)g.kseg;
    const _Float16 *a_src[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int r = slot0 + wave * 32 + t * 8 + srow;
        int ar = g.gather ? g.gather[r] : r;
        ar = ar < 0 ? 0 : ar;
        a_src[t] = g.A + (int64_t)ar * K2 + coff;
    }
    const _Float16 *b_src = g.W + ((int64_t)ex * N + n0 + wave * 32 + srow) * K2 + coff;
    auto stage = [&](int s, int kb) {
        unsigned char *abase = smem + s * MG_STAGE_BYTES + wave * 4096;
        unsigned char *bbase = abase + MG_TILE_BYTES;
        const int koff = kb * MG_BK;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            moe_dma16(a_src[t] + koff, abase + t * 1024);
            moe_dma16(b_src + (int64_t)t * 8 * K2 + koff, bbase + t * 1024);
        }
    };

    // ---- fragment addresses (bytes inside a tile): part p, k quarter fq is logical chunk 4p + fq ----
    const int frow = lane & 15, fq = lane >> 4;
    const int a_row_off = (wm * 64 + frow) * 128;
    const int b_row_off = (wn * 64 + frow) * 128;
    const int chi = ((0 + fq) ^ (lane & 7)) << 4;
    const int clo = ((4 + fq) ^ (lane & 7)) << 4;

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    auto compute = [&](int s) {
        const unsigned char *at = smem + s * MG_STAGE_BYTES;
        const unsigned char *bt = at + MG_TILE_BYTES;
        f16x8 afh[4], afl[4], bfh[4], bfl[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            afh[i] = *reinterpret_cast<const f16x8 *>(at + a_row_off + i * 2048 + chi);
            afl[i] = *reinterpret_cast<const f16x8 *>(at + a_row_off + i * 2048 + clo);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            bfh[j] = *reinterpret_cast<const f16x8 *>(bt + b_row_off + j * 2048 + chi);
            bfl[j] = *reinterpret_cast<const f16x8 *>(bt + b_row_off + j * 2048 + clo);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(afh[i], bfh[j], acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(afl[i], bfh[j], acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(afh[i], bfl[j], acc[i][j], 0, 0, 0);
            }
    };

    // ---- k loop: the DMA of block kb + 1 is issued before the MFMAs of block kb and drained by the barrier behind them ----
    stage(0, 0);
    __syncthreads();   // drains the DMA (vmcnt(0)) and publishes block 0
    int cur = 0;
    for (int kb = 0; kb < nkb - 1; ++kb) {
        stage(cur ^ 1, kb + 1);
        compute(cur);
        __syncthreads();
        cur ^= 1;
    }
    compute(cur);

    // ---- epilogues.  C/D map of the 16x16 MFMA: col = lane & 15, row = (lane >> 4) * 4 + reg ----
    const float oscale = g.scale[ex];
    const float *bias_e = g.bias + (int64_t)ex * N;
    if constexpr (EPI == MG_GELU_PAIR) {
        // fp16 pair out [slots][2N]: the hi parts, then the lo parts, through one LDS patch per wave (whole 128-byte row pieces)
        _Float16 *wreg = reinterpret_cast<_Float16 *>(smem) + wave * (64 * 72);
        _Float16 *out = reinterpret_cast<_Float16 *>(g.out);
#pragma unroll
        for (int part = 0; part < 2; ++part) {
            __syncthreads();
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float bias = bias_e[n0 + wn * 64 + j * 16 + frow];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int rp = 0; rp < 4; rp += 2) {
                        typedef float f32x2 __attribute__((ext_vector_type(2)));
                        typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
                        const f32x2 a = {acc[i][j][rp], acc[i][j][rp + 1]};
                        const f32x2 h = __builtin_elementwise_fma(a, f32x2{oscale, oscale}, f32x2{bias, bias});
                        // QuickGELU, the expression of the dense split epilogue (gemm_f16.hip GE_S_BIAS_GELU)
                        const f32x2 t = h * (-1.702f * 1.44269504088896340736f);
                        const f32x2 d = f32x2{__builtin_amdgcn_exp2f(t[0]), __builtin_amdgcn_exp2f(t[1])} + 1.0f;
                        const f32x2 v = h * f32x2{__builtin_amdgcn_rcpf(d[0]), __builtin_amdgcn_rcpf(d[1])};
                        f16x2 hi, lo;
                        split_pair2(v[0], v[1], hi, lo);
                        wreg[(i * 16 + fq * 4 + rp) * 72 + j * 16 + frow] = part == 0 ? hi[0] : lo[0];
                        wreg[(i * 16 + fq * 4 + rp + 1) * 72 + j * 16 + frow] = part == 0 ? hi[1] : lo[1];
                    }
            }
            __syncthreads();
#pragma unroll
            for (int it = 0; it < 8; ++it) {
                const int lr = it * 8 + (lane >> 3), ch = lane & 7;
                const uint4 v = *reinterpret_cast<const uint4 *>(wreg + lr * 72 + ch * 8);
                *reinterpret_cast<uint4 *>(out + (int64_t)(slot0 + wm * 64 + lr) * (2 * N) + part * N + n0 + wn * 64 + ch * 8) = v;
            }
        }
    } else {
        // fp32 out [slots][N] = acc * s + b: each wave's 64 x 64 block through LDS in two 32-row halves, 256-byte row pieces
        __syncthreads();
        float *wreg = reinterpret_cast<float *>(smem) + wave * (32 * 68);
        float *outp = reinterpret_cast<float *>(g.out);
        const int nbase = n0 + wn * 64, c4 = (lane & 15) * 4;
        const float4 bias4 = *reinterpret_cast<const float4 *>(bias_e + nbase + c4);
#pragma unroll
        for (int half = 0; half < 2; ++half) {
#pragma unroll
            for (int ii = 0; ii < 2; ++ii)
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        wreg[(ii * 16 + fq * 4 + r) * 68 + j * 16 + frow] = acc[half * 2 + ii][j][r];
            __syncthreads();
            const int mbase = slot0 + wm * 64 + half * 32;
#pragma unroll
            for (int it = 0; it < 8; ++it) {
                const int lr = it * 4 + (lane >> 4);
                const float4 a = *reinterpret_cast<const float4 *>(wreg + lr * 68 + c4);
                float4 o;
                o.x = fmaf(a.x, oscale, bias4.x);
                o.y = fmaf(a.y, oscale, bias4.y);
                o.z = fmaf(a.z, oscale, bias4.z);
                o.w = fmaf(a.w, oscale, bias4.w);
                *reinterpret_cast<float4 *>(outp + (int64_t)(mbase + lr) * N + nbase + c4) = o;
            }
            __syncthreads();
        }
    }
}

template <int EPI>
static int moe_gemm_launch(const MoeGemmArgs &g, int64_t rows, hipStream_t stream,
                           int prof_id = EPI == MG_GELU_PAIR ? MPREID_PROF_MOE_FC1 : MPREID_PROF_MOE_FC2) {
    int rc = mpreid_dyn_lds(moe_gemm_kernel<EPI>, (size_t)MG_LDS_BYTES);
    if (rc) return rc;
    void *ptok = mpreid_prof_begin(stream);
    hipLaunchKernelGGL(moe_gemm_kernel<EPI>, dim3((unsigned)((int64_t)g.tiles_max * g.tiles_n)), dim3(256), MG_LDS_BYTES, stream, g);
    mpreid_prof_end(ptok, stream, prof_id, rows, g.N, 2 * g.kseg, 0.0);
    LAUNCH_CHECK();
    return MPREID_OK;
}

// ---------------------------------------------------------------------------------------------
// combine
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void moe_combine_kernel(const float *__restrict__ y, const int *__restrict__ tok_slot,
                                                          const float *__restrict__ tok_w, int64_t rows, int W, int K,
                                                          float *__restrict__ x) {
    const int w4 = W >> 2;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= rows * w4) return;
    const int64_t row = idx / w4;
    const int c = (int)(idx - row * w4) * 4;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int j = 0; j < K; ++j) {   // tok_slot / tok_w hold the row's experts in ascending order
        const int slot = tok_slot[row * K + j];
        if (slot < 0) continue;
        const float wv = tok_w[row * K + j];
        const float4 t = *reinterpret_cast<const float4 *>(y + (int64_t)slot * W + c);
        acc.x = __fadd_rn(acc.x, __fmul_rn(wv, t.x));
        acc.y = __fadd_rn(acc.y, __fmul_rn(wv, t.y));
        acc.z = __fadd_rn(acc.z, __fmul_rn(wv, t.z));
        acc.w = __fadd_rn(acc.w, __fmul_rn(wv, t.w));
    }
    float4 xv = *reinterpret_cast<const float4 *>(x + row * W + c);
    xv.x = xv.x + acc.x;
    xv.y = xv.y + acc.y;
    xv.z = xv.z + acc.z;
    xv.w = xv.w + acc.w;
    *reinterpret_cast<float4 *>(x + row * W + c) = xv;
}

int moe_experts_launch(const _Float16 *a_pairs, const MoeLayout &m, const mpreid_moe_layer *ly, void *ws, float *u_out,
                       hipStream_t stream) {
    char *base = (char *)ws;
    const int W = m.W;
    MoeGemmArgs g{};
    g.tile_tab = (const int2 *)(base + m.tile_tab);
    g.ntiles = (const int *)(base + m.meta);
    g.tiles_max = m.tiles_max;
    // FC1: rows gathered from the LayerNorm pair buffer through the slot table
    g.A = a_pairs;
    g.gather = (const int *)(base + m.slot_row);
    g.W = (const _Float16 *)ly->fc_w;
    g.bias = ly->fc_b;
    g.scale = ly->fc_s;
    g.N = 4 * W;
    g.kseg = W;
    g.tiles_n = g.N / 128;
    int rc;
    if (u_out) {   // the gradient's recompute: the same accumulator through the fp32 epilogue, acc * s + b = the value QuickGELU sees
        g.out = u_out;
        if ((rc = moe_gemm_launch<MG_F32>(g, m.rows, stream, MPREID_PROF_MOE_GRAD_U))) return rc;
    }
    g.out = base + m.hidden;
    if ((rc = moe_gemm_launch<MG_GELU_PAIR>(g, m.rows, stream))) return rc;
    // FC2: slot order in, slot order out
    g.A = (const _Float16 *)(base + m.hidden);
    g.gather = nullptr;
    g.W = (const _Float16 *)ly->proj_w;
    g.bias = ly->proj_b;
    g.scale = ly->proj_s;
    g.N = W;
    g.kseg = 4 * W;
    g.tiles_n = g.N / 128;
    g.out = base + m.y;
    return moe_gemm_launch<MG_F32>(g, m.rows, stream);
}

int moe_mlp_launch(const _Float16 *a_pairs, const MoeLayout &m, const mpreid_moe_layer *ly, float *x, void *ws,
                   hipStream_t stream) {
    char *base = (char *)ws;
    const int W = m.W;
    int rc = moe_experts_launch(a_pairs, m, ly, ws, nullptr, stream);
    if (rc) return rc;
    const int64_t n4 = m.rows * (W / 4);
    void *ptok = mpreid_prof_begin(stream);
    hipLaunchKernelGGL(moe_combine_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, stream, (const float *)(base + m.y),
                       (const int *)(base + m.tok_slot), (const float *)(base + m.tok_w), m.rows, W, m.K, x);
    mpreid_prof_end(ptok, stream, MPREID_PROF_MOE_COMBINE, m.rows, m.E, m.K, 0.0);
    LAUNCH_CHECK();
    return MPREID_OK;
}

// ---------------------------------------------------------------------------------------------
// C ABI: the unit seams
// ---------------------------------------------------------------------------------------------
extern "C" size_t mpreid_moe_workspace_bytes(int64_t rows, int width, int E, int K) {
    if (rows <= 0 || moe_check_shape(rows, width, E, K)) return 0;
    return moe_layout(rows, width, E, K).total;
}

extern "C" int mpreid_moe_route(const float *x, int64_t rows, int width, const float *ln_g, const float *ln_b, const float *gate,
                                int E, int K, int32_t *sel, float *w, float *logits, mpreid_stream_t stream) {
    int rc = moe_check_shape(rows, width, E, K);
    if (rc) return rc;
    ARG_CHECK(x && gate && sel && w && rows > 0);
    ARG_CHECK((ln_g != nullptr) == (ln_b != nullptr));
    ARG_CHECK(((uintptr_t)x & 15) == 0 && ((uintptr_t)gate & 15) == 0 && ((uintptr_t)ln_g & 15) == 0 && ((uintptr_t)ln_b & 15) == 0);
    ARG_CHECK(((uintptr_t)sel & 3) == 0 && ((uintptr_t)w & 3) == 0 && ((uintptr_t)logits & 3) == 0);
    return moe_route_launch(x, rows, width, ln_g, ln_b, gate, E, K, sel, w, logits, (hipStream_t)stream);
}

int moe_check_layer(const mpreid_moe_layer *ly) {
    ARG_CHECK(ly && ly->fc_w && ly->fc_b && ly->proj_w && ly->proj_b && ly->fc_s && ly->proj_s);
    ARG_CHECK(((uintptr_t)ly->fc_w & 15) == 0 && ((uintptr_t)ly->proj_w & 15) == 0 && ((uintptr_t)ly->fc_b & 15) == 0 &&
              ((uintptr_t)ly->proj_b & 15) == 0 && ((uintptr_t)ly->fc_s & 3) == 0 && ((uintptr_t)ly->proj_s & 3) == 0);
    return MPREID_OK;
}

extern "C" int mpreid_moe_mlp_split(const void *a_pairs, int64_t rows, int width, const int32_t *sel, const float *w, int E, int K,
                                    const mpreid_moe_layer *ly, float *x, void *ws, size_t ws_bytes, mpreid_stream_t stream) {
    int rc = moe_check_shape(rows, width, E, K);
    if (rc) return rc;
    ARG_CHECK(a_pairs && sel && w && x && rows > 0);
    if ((rc = moe_check_layer(ly))) return rc;
    ARG_CHECK(((uintptr_t)a_pairs & 15) == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)sel & 3) == 0 && ((uintptr_t)w & 3) == 0);
    ARG_CHECK(((uintptr_t)ws & 255) == 0);
    const MoeLayout m = moe_layout(rows, width, E, K);
    if (!ws || ws_bytes < m.total) {
        mpreid_set_error("MoE workspace too small: %zu < %zu", ws_bytes, m.total);
        return MPREID_ERR_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    if ((rc = moe_dispatch_launch(sel, w, m, ws, s))) return rc;
    return moe_mlp_launch(reinterpret_cast<const _Float16 *>(a_pairs), m, ly, x, ws, s);
}
