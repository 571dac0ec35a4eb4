// rerank_neighbours.hip — re-ranking stages (1)-(6): original_dist, row max + first KR neighbours, reciprocity bits, the
// V rows (utils/reranking.py:33-71).  Shared by the dense and the sparse single call and by the row-sharded phases.
#include "rerank.h"

// ---------------------------------------------------------------------------------------------
// (D + local)^T  /  local^T  (only when local_distmat is given; utils/reranking.py:33-34,43-46)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void make_mt_kernel(const float *__restrict__ D, int64_t ldD,
                                                      const float *__restrict__ local, int64_t N,
                                                      float *__restrict__ MT, int64_t ld) {
    __shared__ float tile[32][33];
    const int64_t bx = (int64_t)blockIdx.x * 32, by = (int64_t)blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5; // 32 x 8
    for (int r = ty; r < 32; r += 8) {
        const int64_t i = by + r, j = bx + tx;
        float v = 0.0f;
        if (i < N && j < N) {
            v = local[i * N + j];
            if (D) v = D[i * ldD + j] + v; // original_dist + local_distmat
        }
        tile[r][tx] = v;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int64_t i = bx + r, j = by + tx; // MT[i][j] = orig[j][i]
        if (i < N && j < N) MT[i * ld + j] = tile[tx][r];
    }
}

// (1) original_dist (the same for DENSE and WIDE)
int launch_original_dist(const float *q, const float *g, int64_t nq, int64_t ng, int d, const float *local, int only_local,
                         float *feat, float *norms, float *D, float *MT, int64_t ld, hipStream_t stream) {
    const int64_t N = nq + ng;
    if (!only_local) {
        HIP_TRY(hipMemcpyAsync(feat, q, (size_t)nq * d * 4, hipMemcpyDeviceToDevice, stream));
        HIP_TRY(hipMemcpyAsync(feat + (size_t)nq * d, g, (size_t)ng * d * 4, hipMemcpyDeviceToDevice, stream));
        int rc = mpreid_sqnorm_f32(feat, N, d, norms, stream);
        if (rc) return rc;
        rc = mpreid_distance_launch(feat, feat, N, N, d, norms, norms, D, ld, 0, stream);
        if (rc) return rc;
    }
    if (local) {
        const dim3 grid((unsigned)((N + 31) / 32), (unsigned)((N + 31) / 32));
        hipLaunchKernelGGL(make_mt_kernel, grid, dim3(256), 0, stream, only_local ? (const float *)nullptr : D, ld, local, N, MT,
                           ld);
        LAUNCH_CHECK();
    }
    return MPREID_OK;
}

// ---------------------------------------------------------------------------------------------
// row max + top-KR selection by (O value, index) ascending; one 256-thread workgroup per row.
// HBM/L2-bound: the row is read 5 times (max, 3 radix histograms, collect); 4*N bytes algorithmic.
// ---------------------------------------------------------------------------------------------
constexpr int TOPK_CAND = 1024;
__global__ __launch_bounds__(256) void rowmax_topk_kernel(const float *__restrict__ MT, int64_t ld, int64_t N, int KR,
                                                          float *__restrict__ rowmax, int *__restrict__ rank,
                                                          const unsigned *__restrict__ row_count) {
    if (row_count && blockIdx.x >= *row_count) return;   // rows past a device-side count (fallback rows) are skipped
    __shared__ unsigned hist[2048];
    __shared__ unsigned long long sel[256];
    __shared__ unsigned long long cand[TOPK_CAND];   // (key, index) of the entries that share the first 22 key bits with
    __shared__ unsigned s_ncand, s_nsel;             // the KR-th smallest, gathered during the last radix pass
    __shared__ float s_red[4];
    __shared__ int s_wave[4];
    __shared__ unsigned s_bin, s_below, s_cnt;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t i = blockIdx.x;
    const float *row = MT + i * ld;
    const int n = (int)N;

    // pass 0: row max (== max over column i of original_dist)
    float mx = -3.402823466e+38f;
    for (int j = tid; j < n; j += 256) mx = fmaxf(mx, row[j]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
    if (lane == 0) s_red[wave] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
    if (tid == 0) rowmax[i] = mx;

    if (tid == 0) {
        s_ncand = 0;
        s_nsel = 0;
    }
    for (int b = tid; b < 256; b += 256) sel[b] = ~0ull;
    // radix select of the KR-th smallest key, 11 + 11 + 10 bits.  The last pass also gathers what the collection
    // needs -- entries below the 22-bit prefix class go straight to the selection, the class itself (normally a few
    // dozen entries) into cand[] -- so that the row is read four times instead of five
    unsigned prefix = 0;
    int kk = KR; // 1-based rank still to find inside the current prefix class
    int bits_done = 0;
    unsigned cnt_eq = 0;
#pragma unroll 1
    for (int pass = 0; pass < 3; ++pass) {
        const int width = (pass == 2) ? 10 : 11;
        const int shift = 32 - bits_done - width;
        const unsigned mask = (1u << width) - 1u;
        for (int b = tid; b < 2048; b += 256) hist[b] = 0;
        __syncthreads();
        for (int j = tid; j < n; j += 256) {
            const unsigned key = fkey(__fdiv_rn(row[j], mx));
            if (bits_done == 0 || (key >> (32 - bits_done)) == prefix) atomicAdd(&hist[(key >> shift) & mask], 1u);
            if (pass == 2) {
                const unsigned top = key >> 10;
                if (top < prefix) {
                    const unsigned p = atomicAdd(&s_nsel, 1u);
                    if (p < 256u) sel[p] = ((unsigned long long)key << 32) | (unsigned)j;
                } else if (top == prefix) {
                    const unsigned p = atomicAdd(&s_ncand, 1u);
                    if (p < (unsigned)TOPK_CAND) cand[p] = ((unsigned long long)key << 32) | (unsigned)j;
                }
            }
        }
        __syncthreads();
        // each thread owns 8 consecutive bins
        unsigned loc[8];
        int sum = 0;
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            loc[b] = hist[tid * 8 + b];
            sum += (int)loc[b];
        }
        int total;
        const int ex = block_excl_scan_256(sum, tid, s_wave, total);
        if (kk > ex && kk <= ex + sum) {
            int run = ex;
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                if (kk > run && kk <= run + (int)loc[b]) {
                    s_bin = (unsigned)(tid * 8 + b);
                    s_below = (unsigned)run;
                    s_cnt = loc[b];
                }
                run += (int)loc[b];
            }
        }
        __syncthreads();
        prefix = (prefix << width) | s_bin;
        kk -= (int)s_below;
        cnt_eq = s_cnt;
        bits_done += width;
        __syncthreads();
    }
    const unsigned T = prefix; // exact key of the KR-th smallest; kk of the cnt_eq equal keys are needed

    // collect (key, index) of the KR selected entries
    const bool from_lds = ((int)cnt_eq == kk) && s_ncand <= (unsigned)TOPK_CAND;
    __syncthreads();
    if (from_lds) {
        // no tie straddles the cut and the prefix class fitted cand[]: everything below the class is in sel[]
        // already, the class contributes its keys <= T; order fixed later by the sort
        const unsigned nc = s_ncand;
        for (unsigned c = tid; c < nc; c += 256) {
            const unsigned long long e = cand[c];
            if ((unsigned)(e >> 32) <= T) {
                const unsigned p = atomicAdd(&s_nsel, 1u);
                if (p < 256u) sel[p] = e;
            }
        }
    } else {
    if (tid == 0) s_cnt = 0;
    for (int b = tid; b < 256; b += 256) sel[b] = ~0ull;
    __syncthreads();
    if ((int)cnt_eq == kk) {
        // no tie straddles the cut: take every key <= T, order fixed later by the sort
        for (int j = tid; j < n; j += 256) {
            const unsigned key = fkey(__fdiv_rn(row[j], mx));
            if (key <= T) {
                const unsigned p = atomicAdd(&s_cnt, 1u);
                if (p < 256u) sel[p] = ((unsigned long long)key << 32) | (unsigned)j;
            }
        }
    } else {
        // ties at the cut: the kk smallest INDICES among the equal keys are taken (ordered scans)
        int run_acc = 0, run_eq = 0;
        for (int j0 = 0; j0 < n; j0 += 256) {
            const int j = j0 + tid;
            unsigned key = 0xffffffffu;
            bool lt = false, eq = false;
            if (j < n) {
                key = fkey(__fdiv_rn(row[j], mx));
                lt = key < T;
                eq = key == T;
            }
            int eq_tot, acc_tot;
            const int eq_rank = run_eq + block_excl_scan_256(eq ? 1 : 0, tid, s_wave, eq_tot);
            const bool accept = lt || (eq && eq_rank < kk);
            const int p = run_acc + block_excl_scan_256(accept ? 1 : 0, tid, s_wave, acc_tot);
            if (accept && p < 256) sel[p] = ((unsigned long long)key << 32) | (unsigned)j;
            run_acc += acc_tot;
            run_eq += eq_tot;
        }
    }
    }
    __syncthreads();
    // bitonic sort of 256 64-bit keys (padding = ~0) ascending => (value, index) order
    for (int size = 2; size <= 256; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            const int partner = tid ^ stride;
            if (partner > tid) {
                const unsigned long long a = sel[tid], b = sel[partner];
                const bool up = ((tid & size) == 0);
                if ((a > b) == up) {
                    sel[tid] = b;
                    sel[partner] = a;
                }
            }
            __syncthreads();
        }
    }
    if (tid < KR) rank[i * KR + tid] = (int)(unsigned)(sel[tid] & 0xffffffffull);
}

// Register-resident variant for N <= 256 * CHUNK: the row is read from HBM exactly once (4*N bytes, the
// algorithmic minimum); every thread keeps its CHUNK orderable keys in VGPRs and the row maximum, the three
// radix-histogram passes and the collection run from registers (+ LDS atomics for the histograms).
template <int CHUNK>
__global__ __launch_bounds__(256) void rowmax_topk_reg_kernel(const float *__restrict__ MT, int64_t ld, int64_t N, int KR,
                                                              float *__restrict__ rowmax, int *__restrict__ rank,
                                                              const unsigned *__restrict__ row_count) {
    if (row_count && blockIdx.x >= *row_count) return;
    __shared__ unsigned long long sel[256];
    __shared__ float s_red[4];
    __shared__ int s_wave[4];
    __shared__ int s_part[8];
    __shared__ unsigned s_cnt;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t i = blockIdx.x;
    const float *row = MT + i * ld;
    const int n = (int)N;

    // register slot s = 4*c4 + e holds element j = c4*1024 + tid*4 + e: 16-byte loads (rows start on 256-byte
    // boundaries: ld is a multiple of 64 floats), every wave instruction moves 1 KB
    static_assert(CHUNK % 4 == 0, "CHUNK must be a multiple of 4");
    float v[CHUNK];
    float mx = -3.402823466e+38f;
#pragma unroll
    for (int c4 = 0; c4 < CHUNK / 4; ++c4) {
        const int j0 = c4 * 1024 + tid * 4;
        float4 f = make_float4(0.f, 0.f, 0.f, 0.f);
        if (j0 + 3 < n) {
            f = *reinterpret_cast<const float4 *>(row + j0);
        } else {
            if (j0 + 0 < n) f.x = row[j0 + 0];
            if (j0 + 1 < n) f.y = row[j0 + 1];
            if (j0 + 2 < n) f.z = row[j0 + 2];
        }
        v[c4 * 4 + 0] = f.x; v[c4 * 4 + 1] = f.y; v[c4 * 4 + 2] = f.z; v[c4 * 4 + 3] = f.w;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (j0 + e < n) mx = fmaxf(mx, v[c4 * 4 + e]);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
    if (lane == 0) s_red[wave] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
    if (tid == 0) rowmax[i] = mx;
    unsigned key[CHUNK];
#pragma unroll
    for (int c = 0; c < CHUNK; ++c) {
        const int j = (c >> 2) * 1024 + tid * 4 + (c & 3);
        key[c] = (j < n) ? fkey(__fdiv_rn(v[c], mx)) : 0xffffffffu;
    }

    // K-th smallest key by bisection on the key value: no atomics (normalised distances share their sign and
    // exponent bits, so radix histograms pile every LDS atomic onto a handful of bins).  Each iteration counts
    // the register-resident keys <= mid and reduces the count over the workgroup; 32 uniform iterations.
    // workgroup sum with ONE barrier per call: partial sums go to alternating slot sets, so a wave that runs
    // ahead writes the other set (it cannot get two calls ahead: it would have to pass the next barrier)
    int bs_phase = 0;
    auto block_sum = [&](int x) -> int {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
        int *slot = s_part + (bs_phase & 1) * 4;
        ++bs_phase;
        if (lane == 0) slot[wave] = x;
        __syncthreads();
        return (slot[0] + slot[1]) + (slot[2] + slot[3]);
    };
    unsigned lo = 0u, hi = 0xfffffffeu; // padded slots hold 0xffffffff and are never counted
#pragma unroll 1
    for (int it = 0; it < 32; ++it) {
        const unsigned mid = lo + ((hi - lo) >> 1);
        int c_le = 0;
#pragma unroll
        for (int c = 0; c < CHUNK; ++c) c_le += (key[c] <= mid) ? 1 : 0;
        if (block_sum(c_le) >= KR) hi = mid; else lo = mid + 1u;
    }
    const unsigned T = lo; // smallest key with count(key <= T) >= KR == the KR-th smallest key
    int c_lt = 0, c_eq = 0;
#pragma unroll
    for (int c = 0; c < CHUNK; ++c) {
        c_lt += (key[c] < T) ? 1 : 0;
        c_eq += (key[c] == T) ? 1 : 0;
    }
    const int cnt_lt = block_sum(c_lt);
    const unsigned cnt_eq = (unsigned)block_sum(c_eq);
    const int kk = KR - cnt_lt; // how many of the cnt_eq keys equal to T are taken
    if (tid == 0) s_cnt = 0;
    sel[tid] = ~0ull;
    __syncthreads();
    if ((int)cnt_eq == kk) {
#pragma unroll
        for (int c = 0; c < CHUNK; ++c) {
            const int j = (c >> 2) * 1024 + tid * 4 + (c & 3);
            if (j < n && key[c] <= T) {
                const unsigned p = atomicAdd(&s_cnt, 1u);
                if (p < 256u) sel[p] = ((unsigned long long)key[c] << 32) | (unsigned)j;
            }
        }
    } else {
        // ties at the cut (rare): the kk smallest INDICES among the equal keys, by ordered scans over
        // index = c*256 + tid.  Keys are recomputed from memory here: indexing the register array with a
        // loop variable would push the whole array into scratch for the common path as well.
        int run_acc = 0, run_eq = 0;
#pragma unroll 1
        for (int c = 0; c < CHUNK; ++c) {
            const int j = c * 256 + tid;
            const bool in = j < n;
            const unsigned kc = in ? fkey(__fdiv_rn(row[j], mx)) : 0xffffffffu;
            const bool lt = in && kc < T, eq = in && kc == T;
            int eq_tot, acc_tot;
            const int eq_rank = run_eq + block_excl_scan_256(eq ? 1 : 0, tid, s_wave, eq_tot);
            const bool accept = lt || (eq && eq_rank < kk);
            const int p = run_acc + block_excl_scan_256(accept ? 1 : 0, tid, s_wave, acc_tot);
            if (accept && p < 256) sel[p] = ((unsigned long long)kc << 32) | (unsigned)j;
            run_acc += acc_tot;
            run_eq += eq_tot;
        }
    }
    __syncthreads();
    if (KR <= 64) {
        // exactly KR <= 64 entries were selected: one wave sorts them with a shuffle-only bitonic network
        if (wave == 0) {
            unsigned long long x = sel[lane];
#pragma unroll
            for (int size = 2; size <= 64; size <<= 1)
#pragma unroll
                for (int stride = size >> 1; stride > 0; stride >>= 1) {
                    const unsigned lo32 = __shfl_xor((unsigned)x, stride, 64);
                    const unsigned hi32 = __shfl_xor((unsigned)(x >> 32), stride, 64);
                    const unsigned long long y = ((unsigned long long)hi32 << 32) | lo32;
                    const bool up = ((lane & size) == 0);
                    const bool lower = ((lane & stride) == 0);
                    // the lower lane of a pair keeps the smaller key in an ascending block, the larger otherwise
                    const bool keep_min = (lower == up);
                    x = keep_min ? (x < y ? x : y) : (x > y ? x : y);
                }
            if (lane < KR) rank[i * KR + lane] = (int)(unsigned)(x & 0xffffffffull);
        }
        return;
    }
    for (int size = 2; size <= 256; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            const int partner = tid ^ stride;
            if (partner > tid) {
                const unsigned long long a = sel[tid], b = sel[partner];
                const bool up = ((tid & size) == 0);
                if ((a > b) == up) {
                    sel[tid] = b;
                    sel[partner] = a;
                }
            }
            __syncthreads();
        }
    }
    if (tid < KR) rank[i * KR + tid] = (int)(unsigned)(sel[tid] & 0xffffffffull);
}

int launch_rowmax_topk(const float *MT, int64_t ld, int64_t N, int KR, int64_t rows, float *rowmax, int *rank,
                       hipStream_t stream, const unsigned *row_count) {
    // measured on MI355X: the register-resident kernel wins for N <= 8192 (0.25 vs 0.34 ms at N = 8000); with 80+
    // keys per thread it drops to 2 waves/SIMD and loses to the radix kernel that re-reads rows from L2
    // (3.3 vs 1.9 ms at N = 20 000)
    const int64_t per = (N + 255) / 256;
    if (per <= 32)
        hipLaunchKernelGGL(rowmax_topk_reg_kernel<32>, dim3((unsigned)rows), dim3(256), 0, stream, MT, ld, N, KR, rowmax, rank,
                           row_count);
    else
        hipLaunchKernelGGL(rowmax_topk_kernel, dim3((unsigned)rows), dim3(256), 0, stream, MT, ld, N, KR, rowmax, rank,
                           row_count);
    LAUNCH_CHECK();
    return MPREID_OK;
}

// ---------------------------------------------------------------------------------------------
// k-reciprocal sets + 2/3-overlap expansion + exp weights -> V row (ELL).  utils/reranking.py:51-71
// (extract_bits_sorted, exact_dist_chain and wave_exact_dists are in rerank.h)
// ---------------------------------------------------------------------------------------------
// MT / rowmax / vcnt / vidx / vval are indexed by the LOCAL row (blockIdx.x); `rank` is the global table and
// row0 the global index of local row 0 (0 on a single GPU; the rank's first row when rows are sharded).
// SPARSE (candidate pipeline, no N x N matrix): the distances of row i to its expansion set are evaluated on the fly
// from the features (exact_dist_chain); MT is unused, feat [N][d] / norms [N] are the inputs.
// ---------------------------------------------------------------------------------------------
// Reciprocity bits of the neighbour table, once per row (they depend on the table only, not on which row's
// expansion asks): for row c and position a < K with n = rank[c][a], p = position of c in rank[n][0..K) or none;
//   bit a of rk[c]  <=>  p exists            (n is a k-reciprocal neighbour of c:        R(c, k1))
//   bit a of rh[c]  <=>  a < h and p < h     (n is a k1/2-reciprocal neighbour of c:     R(c, k1/2))
// utils/reranking.py:53-58 and :61-66 evaluate exactly these with np.where per (row, candidate) pair; done per pair
// on the GPU that was 47 x 26 x 26 scattered 4-byte loads per row and the kernel ran at the texture unit's request
// rate.  RB_WORDS 32-bit words per row and mask (K <= 256).  One wave per row, neighbour rows read 16 bytes per load.
// ---------------------------------------------------------------------------------------------
struct __attribute__((packed, aligned(4))) int4u { int v[4]; };   // 16-byte load from a 4-byte aligned address
__global__ __launch_bounds__(256) void recip_bits_kernel(const int *__restrict__ rank, int64_t N, int K, int KR, int h,
                                                         unsigned *__restrict__ rk, unsigned *__restrict__ rh) {
    const int lane = threadIdx.x & 63;
    const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= N) return;
    for (int a0 = 0; a0 < K; a0 += 64) {
        const int a = a0 + lane;
        int p = -1;
        if (a < K) {
            const int n = rank[c * KR + a];
            const int *row = rank + (int64_t)n * KR;
            int b = 0;
            for (; b + 3 < K; b += 4) {
                const int4u q = *reinterpret_cast<const int4u *>(row + b);
#pragma unroll
                for (int e = 3; e >= 0; --e) p = (q.v[e] == (int)c) ? b + e : p;   // rows hold distinct indices
            }
            for (; b < K; ++b) p = (row[b] == (int)c) ? b : p;
        }
        const unsigned long long mk = __ballot(p >= 0), mh = __ballot(p >= 0 && p < h && a < h);
        if (lane == 0) {
            rk[c * RB_WORDS + (a0 >> 5)] = (unsigned)mk;
            rh[c * RB_WORDS + (a0 >> 5)] = (unsigned)mh;
            if (a0 + 32 < RB_WORDS * 32) {
                rk[c * RB_WORDS + (a0 >> 5) + 1] = (unsigned)(mk >> 32);
                rh[c * RB_WORDS + (a0 >> 5) + 1] = (unsigned)(mh >> 32);
            }
        }
    }
}

// One 256-thread workgroup per row.  (First version: one wave per row walking the expansion candidates one after the
// other -- ~47 iterations of two dependent global loads with 26 active lanes, 130 us per row.  Now a half-wave per
// candidate, eight candidates per iteration.)  Wave 0 keeps the ordered steps (rank-order compaction of R, bitmap
// extraction, numpy-order pairwise sum, ordered write of the V row).
constexpr int KR_HASH_BITS = 9, KR_HASH = 1 << KR_HASH_BITS;   // >= 2 x the largest K (256)
// dynamic LDS of krecip_kernel (the layout at the top of the kernel)
size_t krecip_lds_bytes(bool sparse, int nw, int K, int vcap, int d) {
    size_t b = (size_t)nw * 4 + KR_HASH * 4 + (size_t)K * 8 + (size_t)vcap * 8;
    if (sparse) b += (size_t)K * 4 + (size_t)vcap * 2 + 16 + (size_t)((d + 3) & ~3) * 4 + 64 * WXD_STRIDE * 4;
    return b;
}
// (launch bound: four workgroups per CU = at most 128 VGPRs; unconstrained hipcc took 222 for the rarely taken exact-
// distance path and two workgroups per CU -- 0.53 -> 0.35 ms at N = 20 000 with the bound, 240 B of scratch per lane)
template <bool SPARSE>
__global__ __launch_bounds__(256, 4) void krecip_kernel(const float *__restrict__ MT, int64_t ld, int64_t N,
                                                     const float *__restrict__ rowmax, const int *__restrict__ rank,
                                                     int K, int KR, int h, int vcap, int *__restrict__ vcnt,
                                                     int *__restrict__ vidx, uint16_t *__restrict__ vval, int row0,
                                                     int *__restrict__ r_count,
                                                     const float *__restrict__ feat, const float *__restrict__ norms,
                                                     int d, const float *__restrict__ rankd,
                                                     const unsigned *__restrict__ rk, const unsigned *__restrict__ rh) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int nw = (int)((N + 31) >> 5);
    // LDS (krecip_lds_bytes): the expansion bit mask over all N rows, a 512-slot hash set of R (membership tests of the
    // expansion; a second N-bit mask cost two workgroups per CU at N = 100 000), the lists
    unsigned *Emask = (unsigned *)smem;
    int *Rhash = (int *)(Emask + nw);          // [KR_HASH] open addressing, -1 = empty
    int *fwd = Rhash + KR_HASH;
    int *R = fwd + K;
    int *Elist = R + K;
    float *wbuf = (float *)(Elist + vcap);
    // SPARSE only: exact distances of the first K neighbours (from the refinement), the indices of expansion entries
    // that are not among them, row i of feat and the wave_exact_dists tile (16-byte aligned)
    float *fdist = wbuf + vcap;
    uint16_t *miss = (uint16_t *)(fdist + K);  // positions in Elist (< vcap < 65536)
    float *qrow = reinterpret_cast<float *>((reinterpret_cast<uintptr_t>(miss + vcap) + 15) & ~(uintptr_t)15);
    float *xtile = qrow + ((d + 3) & ~3);
    auto rh_slot = [](int f) -> unsigned { return ((unsigned)f * 2654435761u) >> (32 - KR_HASH_BITS); };
    __shared__ int s_nR, s_nE, s_nmiss;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = blockIdx.x;      // local row
    const int i = row0 + li;        // global row

    for (int w = tid; w < nw; w += 256) Emask[w] = 0u;
    for (int w = tid; w < KR_HASH; w += 256) Rhash[w] = -1;
    for (int a = tid; a < K; a += 256) {
        fwd[a] = rank[(int64_t)i * KR + a];
        if (SPARSE) fdist[a] = rankd[(int64_t)i * KR + a];
    }
    if (tid == 0) s_nmiss = 0;
    __syncthreads();

    // k_reciprocal_index: fwd[a] such that i is among the first K neighbours of fwd[a]; rank order kept (wave 0)
    if (wave == 0) {
        int nR = 0;
        for (int a0 = 0; a0 < K; a0 += 64) {
            const int a = a0 + lane;
            bool f = false;
            int c = -1;
            if (a < K) {
                c = fwd[a];
                f = (rk[(int64_t)i * RB_WORDS + (a >> 5)] >> (a & 31)) & 1u;
            }
            const unsigned long long m = __ballot(f);
            if (f) {
                const int pos = nR + __popcll(m & ((1ull << lane) - 1ull));
                R[pos] = c;
                for (unsigned sl = rh_slot(c);; sl = (sl + 1) & (KR_HASH - 1)) {   // (the entries of a rank row are distinct)
                    if (atomicCAS(&Rhash[sl], -1, c) == -1) break;
                }
                atomicOr(&Emask[c >> 5], 1u << (c & 31));
            }
            nR += __popcll(m);
        }
        if (lane == 0) {
            s_nR = nR;
            if (r_count) r_count[li] = nR;   // |R(i, k1)|, summed afterwards (statistics)
        }
    }
    __syncthreads();
    const int nR = s_nR;

    // expansion: the k/2-reciprocal set of every candidate, accepted on > 2/3 overlap with R.  A half-wave (32
    // lanes) per candidate; h <= 32 entries are tested in one step, larger h in chunks of 32.
    {
        const int half = tid >> 5, hl = tid & 31;          // 8 half-waves
        const unsigned long long hmask = (hl == (lane & 31) && (lane & 32)) ? 0xffffffff00000000ull : 0x00000000ffffffffull;
        for (int a0 = 0; a0 < nR; a0 += 8) {
            const int a = a0 + half;
            const bool live = a < nR;
            const int cand = live ? R[a] : 0;
            const int *cf = rank + (int64_t)cand * KR;
            int nRc = 0, inter = 0;
            unsigned okbits = 0u;
            for (int b0 = 0, ch = 0; b0 < h; b0 += 32, ++ch) {
                const int b = b0 + hl;
                bool ok = false, inr = false;
                if (live && b < h) {
                    ok = (rh[(int64_t)cand * RB_WORDS + (b >> 5)] >> (b & 31)) & 1u;
                    if (ok) {
                        const int f = cf[b];
                        for (unsigned sl = rh_slot(f);; sl = (sl + 1) & (KR_HASH - 1)) {
                            const int hv = Rhash[sl];
                            if (hv == f) inr = true;
                            if (hv == f || hv == -1) break;
                        }
                    }
                }
                nRc += __popcll(__ballot(ok) & hmask);
                inter += __popcll(__ballot(inr) & hmask);
                if (ok) okbits |= (1u << ch);
            }
            if (live && (double)inter > (2.0 / 3.0) * (double)nRc) {
                for (int b0 = 0, ch = 0; b0 < h; b0 += 32, ++ch) {
                    const int b = b0 + hl;
                    if (b < h && ((okbits >> ch) & 1u)) {
                        const int f = cf[b];
                        atomicOr(&Emask[f >> 5], 1u << (f & 31));
                    }
                }
            }
        }
    }
    __syncthreads();

    // np.unique(expansion index) == set bits of Emask in ascending order
    if (wave == 0) {
        const int n = extract_bits_sorted(Emask, nw, Elist, lane);
        if (lane == 0) s_nE = n;
    }
    if (SPARSE)
        for (int k = tid; k < d; k += 256) qrow[k] = feat[(int64_t)i * d + k];
    __syncthreads();
    const int nE = s_nE;
    const float mx = rowmax[li];
    if (SPARSE) {
        // entries among the first K neighbours (all of R, i.e. nearly everything) have their exact distance already;
        // the others are evaluated now
        for (int t = tid; t < nE; t += 256) {
            const int j = Elist[t];
            int pos = -1;
            for (int a = 0; a < K; ++a) pos = (fwd[a] == j) ? a : pos;
            if (pos >= 0) {
                wbuf[t] = mpreid_np_expf(-__fdiv_rn(fdist[pos], mx));
            } else {
                miss[atomicAdd(&s_nmiss, 1)] = (uint16_t)t;
            }
        }
        __syncthreads();
        const int nmiss = s_nmiss;
        if (wave == 0 && nmiss > 0) {
            const float ni = norms[i];
            for (int t0 = 0; t0 < nmiss; t0 += 64) {
                const int u = t0 + lane;
                const int t = u < nmiss ? (int)miss[u] : -1;
                const float dij = wave_exact_dists(qrow, feat, d, t >= 0 ? Elist[t] : -1, ni, norms, xtile, lane);
                if (t >= 0) wbuf[t] = mpreid_np_expf(-__fdiv_rn(dij, mx));
            }
        }
    } else {
        const float *row = MT + (int64_t)li * ld;
        for (int t = tid; t < nE; t += 256) wbuf[t] = mpreid_np_expf(-__fdiv_rn(row[Elist[t]], mx));
    }
    __syncthreads();
    if (wave != 0) return;
    const float s = wave_pairwise_sum(wbuf, nE, lane);
    // V[i, E] = fp16(weight / sum); only non-zero halves are kept (V != 0 tests later)
    int out = 0;
    for (int t0 = 0; t0 < nE; t0 += 64) {
        const int t = t0 + lane;
        uint16_t hv = 0;
        if (t < nE) hv = h_from_f32(__fdiv_rn(wbuf[t], s));
        const bool nz = (hv & 0x7fffu) != 0;
        const unsigned long long m = __ballot(nz);
        if (nz) {
            const int p = out + __popcll(m & ((1ull << lane) - 1ull));
            vidx[(int64_t)li * vcap + p] = Elist[t];
            vval[(int64_t)li * vcap + p] = hv;
        }
        out += __popcll(m);
    }
    if (lane == 0) vcnt[li] = out;
}

// (4)-(6) V rows of the rows [row0, row0 + rows) of the N x N problem: the reciprocity bits of ALL rows into rk
// (mpreid_rr_krecip_scratch_bytes; the candidates of a row live anywhere), then the k-reciprocal kernel.  Dense: MT /
// rowmax / vcnt.. are indexed by the local row, feat = norms = rankd = NULL, d = 0.  sparse: distances on the fly from
// feat / norms, rankd indexed by the GLOBAL row.  r_count: |R| per row, or NULL.
int launch_krecip(bool sparse, const float *MT, int64_t ld, int64_t N, const float *rowmax, const int *rank, int K, int KR,
                  int h, int vcap, int *vcnt, int *vidx, uint16_t *vval, int64_t row0, int64_t rows, int *r_count,
                  const float *feat, const float *norms, int d, const float *rankd, unsigned *rk, hipStream_t stream) {
    const auto kernel = sparse ? krecip_kernel<true> : krecip_kernel<false>;
    const size_t lds = krecip_lds_bytes(sparse, (int)((N + 31) >> 5), K, vcap, d);
    if (lds > LDS_WG_MAX) {   // an error that names the limit in the caller's terms (include/mpreid.h "Limits")
        mpreid_set_error("re_ranking: k1 = %d at N = %lld needs %zu bytes of LDS for the expansion lists of one row; the limit is "
                         "160 KiB per workgroup (k1 <= ~190 at N >= 20000, k1 <= 255 for N <= 18000; include/mpreid.h). The "
                         "reference (utils/reranking.py:29) takes any k1 and is called with k1 = 50",
                         K - 1, (long long)N, lds);
        return MPREID_ERR_UNSUPPORTED;
    }
    int rc = mpreid_dyn_lds(kernel, lds);
    if (rc) return rc;
    unsigned *rh = rk + (size_t)N * RB_WORDS;
    hipLaunchKernelGGL(recip_bits_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, stream, rank, N, K, KR, h, rk, rh);
    hipLaunchKernelGGL(kernel, dim3((unsigned)rows), dim3(256), lds, stream, MT, ld, N, rowmax, rank, K, KR, h, vcap, vcnt, vidx,
                       vval, (int)row0, r_count, feat, norms, d, rankd, rk, rh);
    LAUNCH_CHECK();
    return MPREID_OK;
}
