// rerank_sparse.hip — the candidate pipeline of the re-ranking: its kernels, its two host halves (cand_lists / cand_refine:
// all rows in the single call, a row block in the sharded phase 1 of rerank.hip) and the single-call driver.
#include "rerank.h"

// =============================================================================================
// Candidate pipeline ("sparse" algorithm): initial_rank and the column maxima WITHOUT the N x N matrix.
//
//   1. feat -> fp16 (one rounding per element); every 16th row forms a sample.
//   2. sample pass: d~ = one-pass fp16 distances of every row against the sample ([N][N/16] fp32, 1/16 of N x N);
//      per row the r-th smallest and the largest sample value give two thresholds (rr2_threshold_kernel).
//   3. fused pass: the full symmetric fp16 GEMM on the matrix cores with the GE_CAND epilogue (gemm_f16.hip):
//      nothing is stored, entries with d~ <= tlo[i] or d~ >= thi[i] are appended to row i's candidate lists
//      (~160 + ~16 of N entries).
//   4. refinement (rr2_refine_kernel): the EXACT distance (exact_dist_chain = the oracle's fmaf chain) of the few
//      candidates that can still be among the first KR neighbours / be the row maximum, then the exact selection by
//      (O value, index).  Everything rests on one bound:   |d~ - d_exact| <= eps_i   (derivation at rr2_eps).
//      A row whose candidate list cannot be PROVEN to contain the answer (too few / too many candidates, threshold
//      closer than 2 eps to the KR-th candidate) is handed to the fallback: its whole distance row is computed
//      exactly and selected by the dense kernel.  So the result is always the dense algorithm's, bit for bit;
//      the thresholds only decide how much work that takes.
//   5. k-reciprocal expansion with on-the-fly exact distances (krecip_kernel<true>), query expansion, inverted index
//      as before; the Jaccard stage reads the exact distance rows of the QUERIES only ([nq][N]).
// HBM traffic: N x N/16 fp32 once, instead of N x N fp32 written once and read ~5 times.
// =============================================================================================

// |fp16 one-pass distance - exact fp32-chain distance| for rows i, j with norms a = |f_i|, b = |f_j|, dimension D:
//   inputs rounded to fp16: relative 2^-11 each  ->  |dot~ - dot| <= (2 * 2^-11 + 2^-22) * sum |x_k y_k| <= 2^-10 * 1.001 * a * b
//   fp16 subnormals (|x_k| < 2^-14): absolute 2^-25 per element  ->  <= 2^-25 * sqrt(D) * (a + b)
//   fp32 accumulation, either side, any order: <= D * 2^-24 * a * b each
//   d = fmaf(-2, dot, a^2 + b^2): the dot errors double; the norm sum and the final rounding add 2^-23 * (a^2 + b^2 + 2ab)
// eps_i uses b <= G = the largest row norm.
__device__ __forceinline__ float rr2_eps(float a, float G, int D) {
    const float ab = a * G;
    return ab * (0.0019551f + 2.4e-7f * (float)D) + 1.2e-7f * sqrtf((float)D) * (a + G) + 2.4e-7f * (a + G) * (a + G);
}

// rows r*stride of x (fp32 [n][d]) -> fp16 [n_out_pad][d_pad], zero padded; norms gathered alongside (padded with 0)
__global__ __launch_bounds__(256) void rr2_cast_rows_kernel(const float *__restrict__ x, const float *__restrict__ sqn,
                                                            int64_t n, int d, int stride, _Float16 *__restrict__ y,
                                                            int d_pad, float *__restrict__ sqn_out) {
    const int64_t r = blockIdx.x, src = r * stride;
    const bool ok = src < n;
    for (int k = threadIdx.x; k < d_pad; k += 256) y[r * (int64_t)d_pad + k] = (ok && k < d) ? (_Float16)x[src * d + k] : (_Float16)0.0f;
    if (sqn_out && threadIdx.x == 0) sqn_out[r] = ok ? sqn[src] : 0.0f;
}

// G = max row norm -> gstat[0]; gstat[1] = 1 if any norm is too large for fp16 operands (or not finite)
__global__ __launch_bounds__(1024) void rr2_norm_stats_kernel(const float *__restrict__ sqn, int64_t n, float *__restrict__ gstat) {
    __shared__ float red[16];
    __shared__ int bad_any;
    if (threadIdx.x == 0) bad_any = 0;
    __syncthreads();
    float m = 0.0f;
    int bad = 0;   // fmaxf DROPS a NaN operand, so non-finite norms are tracked explicitly (a NaN row must not pass)
    for (int64_t i = threadIdx.x; i < n; i += 1024) {
        const float v = sqn[i];
        bad |= !(v >= 0.0f && v < 3.0e38f);
        m = fmaxf(m, v);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    if (bad) atomicOr(&bad_any, 1);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 16; ++w) m = fmaxf(m, red[w]);
        const float G = sqrtf(m);
        gstat[0] = G;
        gstat[1] = (G < 3.0e4f && !bad_any) ? 0.0f : 1.0f;
    }
}

// per row: thresholds from the sample distances.  tlo = r-th smallest sample value (about 16 r of the N entries of
// the row lie below it), thi = sample maximum - 2 eps.  Padded rows get -inf / +inf.  256 threads per row.
__global__ __launch_bounds__(256) void rr2_threshold_kernel(const float *__restrict__ S, int64_t ldS, int ns, int64_t N,
                                                            int rsel, const float *__restrict__ sqn,
                                                            const float *__restrict__ gstat, int D,
                                                            float *__restrict__ tlo, float *__restrict__ thi,
                                                            float *__restrict__ eps, unsigned *__restrict__ cnt_lo,
                                                            unsigned *__restrict__ cnt_hi) {
    __shared__ unsigned keys[512];
    __shared__ float s_red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t i = blockIdx.x;
    if (tid == 0) {
        cnt_lo[i] = 0u;
        cnt_hi[i] = 0u;
    }
    if (i >= N) {
        if (tid == 0) {
            tlo[i] = -__builtin_huge_valf();
            thi[i] = __builtin_huge_valf();
            eps[i] = 0.0f;
        }
        return;
    }
    const float *row = S + i * ldS;
    // A threshold is all this has to produce (correctness never depends on it), so the selection is approximate and
    // cheap: every thread keeps the minimum of its strided slice, each wave sorts its 64 minima with a shuffle-only
    // bitonic network, and the r-th smallest of the four waves' r smallest is taken.  It is >= the row's true r-th
    // smallest sample value (two of the r smallest in one thread's slice hide one of them), which only adds candidates.
    unsigned k0 = 0xffffffffu;
    float mx = -3.402823466e+38f;
    for (int j = tid; j < ns; j += 256) {
        const float v = row[j];
        mx = fmaxf(mx, v);
        const unsigned k = fkey(v);
        k0 = k < k0 ? k : k0;
    }
#pragma unroll
    for (int size = 2; size <= 64; size <<= 1)
#pragma unroll
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            const unsigned y = __shfl_xor(k0, stride, 64);
            const bool keep_min = (((lane & stride) == 0) == ((lane & size) == 0));
            k0 = keep_min ? (k0 < y ? k0 : y) : (k0 > y ? k0 : y);
        }
    if (lane < 16) keys[wave * 16 + lane] = k0;          // the wave's 16 smallest minima, ascending
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
    if (lane == 0) s_red[wave] = mx;
    __syncthreads();
    if (wave == 0) {
        unsigned x = keys[lane];                          // 4 x 16 keys
#pragma unroll
        for (int size = 2; size <= 64; size <<= 1)
#pragma unroll
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                const unsigned y = __shfl_xor(x, stride, 64);
                const bool keep_min = (((lane & stride) == 0) == ((lane & size) == 0));
                x = keep_min ? (x < y ? x : y) : (x > y ? x : y);
            }
        keys[lane] = x;
    }
    __syncthreads();
    if (tid == 0) {
        int r = rsel < ns ? rsel : ns;
        r = r < 16 ? r : 16;
        const unsigned kk = keys[r - 1];
        const unsigned u = (kk & 0x80000000u) ? (kk & 0x7fffffffu) : ~kk;   // inverse of fkey
        const float e = rr2_eps(sqrtf(sqn[i]), gstat[0], D);
        tlo[i] = __uint_as_float(u);
        thi[i] = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3])) - 2.0f * e;
        eps[i] = e;
    }
}

// Refinement of one row (256 threads): see the header of this section.  status[i]: 0 = certified, 1 = fallback.
constexpr int RR2_MAXE = 128;   // exact evaluations per row on the `lo` side
constexpr int RR2_MAXH = 32;    // ... and on the `hi` side
template <int CAP_LO, int CAP_HI>
__global__ __launch_bounds__(256) void rr2_refine_kernel(const float *__restrict__ feat, const float *__restrict__ sqn,
                                                         int64_t N, int d, int KR, const unsigned *__restrict__ cnt_lo,
                                                         const uint2 *__restrict__ list_lo,
                                                         const unsigned *__restrict__ cnt_hi,
                                                         const uint2 *__restrict__ list_hi,
                                                         const float *__restrict__ tlo, const float *__restrict__ eps,
                                                         float *__restrict__ rowmax, int *__restrict__ rank,
                                                         float *__restrict__ rankd,
                                                         unsigned *__restrict__ fb_count, int *__restrict__ fb_rows,
                                                         unsigned fb_max, int64_t row0) {
    // lists, thresholds, rank / rankd / rowmax and the fallback list are indexed by the LOCAL row (blockIdx.x); feat
    // and sqn are the global arrays and row0 the global index of local row 0 (0 unless the rows are sharded)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    static_assert(CAP_LO <= 512 && CAP_HI <= 256, "list capacities");
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(smem);   // [512]
    unsigned long long *ekey = keys + 512;                                     // [RR2_MAXE] exact (O key, index)
    int *hsel = reinterpret_cast<int *>(ekey + RR2_MAXE);                      // [RR2_MAXH]
    float *hval = reinterpret_cast<float *>(hsel + RR2_MAXH);                  // [RR2_MAXH]
    float *qrow = hval + RR2_MAXH;                                             // [d rounded up to 4]
    float *xtile = qrow + ((d + 3) & ~3);                                      // [2 waves][64][WXD_STRIDE]
    __shared__ float s_red[4];
    __shared__ unsigned s_cnt;
    __shared__ int s_fail;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t i = blockIdx.x;
    const unsigned nlo = cnt_lo[i], nhi = cnt_hi[i];
    const float e = eps[i];
    if (tid == 0) {
        s_cnt = 0u;
        s_fail = (nlo > (unsigned)CAP_LO || nhi > (unsigned)CAP_HI || nlo < (unsigned)KR || nhi < 1u) ? 1 : 0;
    }
    for (int k = tid; k < d; k += 256) qrow[k] = feat[(row0 + i) * d + k];
    // ---- lo side: sort the candidates by approximate distance ----
    for (int t = tid; t < 512; t += 256) {
        unsigned long long kv = ~0ull;
        if (t < (int)nlo && t < CAP_LO) {
            const uint2 c = list_lo[i * CAP_LO + t];
            kv = ((unsigned long long)fkey(__uint_as_float(c.y)) << 32) | c.x;
        }
        keys[t] = kv;
    }
    __syncthreads();
    const bool fail0 = s_fail != 0;
    if (!fail0) {
        const int sort_n = nlo <= 256u ? 256 : 512;   // (most rows have ~160 candidates)
        for (int size = 2; size <= sort_n; size <<= 1)
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int a_i = tid + h * 256, partner = a_i ^ stride;
                    if (a_i < sort_n && partner > a_i) {
                        const unsigned long long a = keys[a_i], b = keys[partner];
                        const bool up = ((a_i & size) == 0);
                        if ((a > b) == up) {
                            keys[a_i] = b;
                            keys[partner] = a;
                        }
                    }
                }
                __syncthreads();
            }
    }
    // x~ = KR-th smallest approximate distance; every candidate up to x~ + 2 eps is evaluated exactly
    float xt = 0.0f, cut = 0.0f;
    int m = 0;
    if (!fail0) {
        const unsigned kx = (unsigned)(keys[KR - 1] >> 32);
        xt = __uint_as_float((kx & 0x80000000u) ? (kx & 0x7fffffffu) : ~kx);
        cut = xt + 2.0f * e;
        const unsigned kcut = fkey(cut);
        // count of keys <= cut (keys sorted ascending; nlo <= 512)
        int c = 0;
        for (int t = tid; t < (int)nlo; t += 256) c += ((unsigned)(keys[t] >> 32) <= kcut) ? 1 : 0;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off, 64);
        if (lane == 0) atomicAdd(&s_cnt, (unsigned)c);
    }
    __syncthreads();
    m = (int)s_cnt;
    __syncthreads();
    // certification 1: everything that was NOT a candidate has d~ > tlo, so exact > tlo - eps; it must lie above the
    // exact KR-th, which is <= x~ + eps  ->  x~ + 2 eps <= tlo;  and the evaluation budget
    if (tid == 0) {
        if (!fail0 && (m > RR2_MAXE || !(xt + 2.0f * e <= tlo[i]))) s_fail = 1;
        s_cnt = 0u;
    }
    // ---- hi side: approximate maximum, everything within 2 eps of it is evaluated exactly ----
    float hm = -3.402823466e+38f;
    if (!fail0)
        for (int t = tid; t < (int)nhi; t += 256) hm = fmaxf(hm, __uint_as_float(list_hi[i * CAP_HI + t].y));
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) hm = fmaxf(hm, __shfl_xor(hm, off, 64));
    if (lane == 0) s_red[wave] = hm;
    __syncthreads();
    hm = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
    if (!fail0)
        for (int t = tid; t < (int)nhi; t += 256) {
            const uint2 c = list_hi[i * CAP_HI + t];
            if (__uint_as_float(c.y) >= hm - 2.0f * e) {
                const unsigned p = atomicAdd(&s_cnt, 1u);
                if (p < (unsigned)RR2_MAXH) hsel[p] = (int)c.x;
            }
        }
    __syncthreads();
    const int mh = (int)s_cnt;
    if (tid == 0 && (mh > RR2_MAXH || m + mh > RR2_MAXE)) s_fail = 1;   // lo and hi evaluations share 128 lanes
    __syncthreads();
    if (s_fail) {
        if (tid == 0) {
            const unsigned p = atomicAdd(fb_count, 1u);
            if (p < fb_max) fb_rows[p] = (int)i;
        }
        return;
    }
    // ---- exact distances: threads 0..m-1 the lo candidates, threads m..m+mh-1 the hi candidates (two waves) ----
    const float ni = sqn[row0 + i];
    float dex = 0.0f;
    int jx = -1;
    if (tid < m) jx = (int)(unsigned)(keys[tid] & 0xffffffffull);
    else if (tid < m + mh) jx = hsel[tid - m];
    if (wave < 2 && wave * 64 < m + mh)   // wave-uniform
        dex = wave_exact_dists(qrow, feat, d, jx, ni, sqn, xtile + wave * 64 * WXD_STRIDE, lane);
    if (tid >= m && tid < m + mh) hval[tid - m] = dex;
    __syncthreads();
    float mx = -3.402823466e+38f;
    for (int t = 0; t < mh; ++t) mx = fmaxf(mx, hval[t]);   // exact row maximum (see the header: always certified)
    // ---- exact selection by (O value, index) ----
    if (tid < RR2_MAXE) ekey[tid] = (tid < m) ? (((unsigned long long)fkey(__fdiv_rn(dex, mx)) << 32) | (unsigned)jx) : ~0ull;
    // the approximate keys are done with (every thread has read its jx before the barrier above): their memory now
    // holds (index, exact distance) by slot, for the distances of the selected neighbours written out below
    int *djx = reinterpret_cast<int *>(keys);
    float *dlo = reinterpret_cast<float *>(keys + 64);
    if (tid < m) {
        djx[tid] = jx;
        dlo[tid] = dex;
    }
    __syncthreads();
    for (int size = 2; size <= RR2_MAXE; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            if (tid < RR2_MAXE) {
                const int partner = tid ^ stride;
                if (partner > tid) {
                    const unsigned long long a = ekey[tid], b = ekey[partner];
                    const bool up = ((tid & size) == 0);
                    if ((a > b) == up) {
                        ekey[tid] = b;
                        ekey[partner] = a;
                    }
                }
            }
            __syncthreads();
        }
    // certification 2 (ties after the division): whatever was not evaluated has exact distance > x~ + eps (the
    // unevaluated candidates) or > tlo - eps >= x~ + eps (the rest); its O value is >= fdiv(x~ + eps, mx), which
    // must be STRICTLY above the KR-th selected O value
    const unsigned okx = (unsigned)(ekey[KR - 1] >> 32);
    const bool ok = fkey(__fdiv_rn(xt + e, mx)) > okx;
    if (!ok) {
        if (tid == 0) {
            const unsigned p = atomicAdd(fb_count, 1u);
            if (p < fb_max) fb_rows[p] = (int)i;
        }
        return;
    }
    if (tid < KR) {
        const int j = (int)(unsigned)(ekey[tid] & 0xffffffffull);
        rank[i * KR + tid] = j;
        float dj = 0.0f;   // D[i][j], exact: the expansion kernel weighs the neighbours with exp(-D / rowmax)
        for (int sl = 0; sl < m; ++sl) dj = (djx[sl] == j) ? dlo[sl] : dj;
        rankd[i * KR + tid] = dj;
    }
    if (tid == 0) rowmax[i] = mx;
}

// fallback rows: gather their features / norms, and scatter their dense results back
__global__ __launch_bounds__(256) void rr2_fb_gather_kernel(const float *__restrict__ feat, const float *__restrict__ sqn, int d,
                                                            const int *__restrict__ fb_rows,
                                                            const unsigned *__restrict__ fb_count, unsigned fb_max,
                                                            float *__restrict__ fb_feat, float *__restrict__ fb_sqn,
                                                            int64_t row0) {
    const unsigned b = blockIdx.x;
    const unsigned cnt = *fb_count < fb_max ? *fb_count : fb_max;
    if (b >= cnt) return;
    const int64_t i = row0 + fb_rows[b];
    for (int k = threadIdx.x; k < d; k += 256) fb_feat[(int64_t)b * d + k] = feat[i * d + k];
    if (threadIdx.x == 0) fb_sqn[b] = sqn[i];
}
__global__ __launch_bounds__(256) void rr2_fb_scatter_kernel(const int *__restrict__ fb_rows, const unsigned *__restrict__ fb_count,
                                                             unsigned fb_max, const float *__restrict__ fb_rowmax,
                                                             const int *__restrict__ fb_rank, int KR,
                                                             const float *__restrict__ fb_D, int64_t ld,
                                                             float *__restrict__ rowmax, int *__restrict__ rank,
                                                             float *__restrict__ rankd) {
    const unsigned b = blockIdx.x;
    const unsigned cnt = *fb_count < fb_max ? *fb_count : fb_max;
    if (b >= cnt) return;
    const int64_t i = fb_rows[b];
    for (int t = threadIdx.x; t < KR; t += 256) {
        const int j = fb_rank[(int64_t)b * KR + t];
        rank[i * KR + t] = j;
        rankd[i * KR + t] = fb_D[(int64_t)b * ld + j];
    }
    if (threadIdx.x == 0) rowmax[i] = fb_rowmax[b];
}

// ---- host side ----
constexpr int RR2_CAP_LO = 384, RR2_CAP_HI = 128, RR2_SAMPLE_STRIDE = 16, RR2_RSEL = 10, RR2_QCAP = 4096;

CandBuffers take_cand_buffers(WsCursor &take, int64_t n, int d, int64_t rows, int kr, int64_t slack) {
    CandBuffers c{};
    c.Np = (int64_t)align_up((size_t)n, 256);
    c.Nsp = (int64_t)align_up((size_t)((n + RR2_SAMPLE_STRIDE - 1) / RR2_SAMPLE_STRIDE), 256);
    c.Mp = (int64_t)align_up((size_t)rows, 256);
    c.slack = slack;
    c.ld = (int64_t)align_up((size_t)n, 64);
    c.dp = (int)align_up((size_t)d, 64);
    c.fb_max = std::max<int64_t>(256, rows / 16);
    const size_t Np = (size_t)(c.Np + slack), Mp = (size_t)c.Mp, F = (size_t)c.fb_max;
    c.sqn = take(Np * 4);
    c.feat16 = take(Np * (size_t)c.dp * 2);
    c.samp16 = take((size_t)c.Nsp * c.dp * 2);
    c.sampn = take((size_t)c.Nsp * 4);
    c.sampD = take(Mp * (size_t)c.Nsp * 4);
    c.tlo = take(Mp * 4);
    c.thi = take(Mp * 4);
    c.eps = take(Mp * 4);
    c.cnt_lo = take(Mp * 4);
    c.cnt_hi = take(Mp * 4);
    c.list_lo = take(Mp * (size_t)RR2_CAP_LO * 8);
    c.list_hi = take(Mp * (size_t)RR2_CAP_HI * 8);
    c.gstat = take(64);
    c.fb_count = take(64);
    c.fb_rows = take(F * 4);
    c.fb_feat = take(F * (size_t)d * 4);
    c.fb_sqn = take(F * 4);
    c.fb_D = take(F * (size_t)c.ld * 4);
    c.fb_rowmax = take(F * 4);
    c.fb_rank = take(F * (size_t)kr * 4);
    return c;
}

Rerank2Layout make_layout2(int64_t nq, int64_t ng, int d, int k1, int k2, bool split3_rows) {
    Rerank2Layout L{};
    L.N = nq + ng;
    L.ld = (int64_t)align_up((size_t)L.N, 64);
    static_cast<RerankK &>(L) = clamp_k(L.N, k1, k2);
    L.qcap_bound = std::min<int64_t>(L.qcap_bound, RR2_QCAP);
    WsCursor take;
    const size_t N = (size_t)L.N;
    L.feat = take(N * (size_t)d * 4);
    L.c = take_cand_buffers(take, L.N, d, L.N, L.KR, 0);
    L.rowmax = take(N * 4);
    L.rank = take(N * (size_t)L.KR * 4);
    L.rankd = take(N * (size_t)L.KR * 4);
    L.rbits = take(N * (size_t)RB_WORDS * 4 * 2);
    L.vcnt = take(N * 4);
    L.vidx = take(N * (size_t)L.vcap * 4);
    L.vval = take(N * (size_t)L.vcap * 2);
    L.ucnt = take(N * 4);
    L.qcnt = take(N * 4);
    L.qidx = take(N * (size_t)L.qcap_bound * 4);
    L.qval = take(N * (size_t)L.qcap_bound * 2);
    L.ccnt = take((N + 1) * 4);
    L.chist = take(csc_hist_bytes((int64_t)N));   // CSC_B block histograms + chunk bounds
    L.cptr = take((N + 1) * 8);
    L.crow = take(N * (size_t)L.qcap_bound * 4);
    L.cval = take(N * (size_t)L.qcap_bound * 2);
    L.dq = take((size_t)nq * L.ld * 4);
    L.counters = take(64);
    L.dq_ws_bytes = split3_rows ? mpreid_distance_split3_ws_bytes(nq, ng, d) : 0;
    L.dq_ws = take(L.dq_ws_bytes);
    L.total = take.off;
    return L;
}

// the sparse algorithm applies when there is no local_distmat, the problem is large enough for the sample to mean
// something, and the neighbour count fits the refinement kernel's evaluation budget
bool sparse_eligible(int64_t nq, int64_t ng, int k1, int k2, const float *local) {
    const int64_t N = nq + ng;
    return local == nullptr && N >= 2048 && clamp_k(N, k1, k2).KR <= 64;
}

// First half of the pipeline for the rows [r_lo, r_lo + rows): fp16 operands of ALL rows (every row block needs all
// columns) and of the sample, sample pass and thresholds for the block, candidate GEMM block x all columns.  sym = 1 only
// for the whole square (no symmetry to exploit inside a row block); stagger: a timing experiment of the GEMM, 0 otherwise.
int cand_lists(const float *feat, char *ws, const CandBuffers &c, int64_t n, int d, int64_t r_lo, int64_t rows, int sym,
               int stagger, hipStream_t stream) {
    float *sqn = (float *)(ws + c.sqn);
    _Float16 *feat16 = (_Float16 *)(ws + c.feat16), *samp16 = (_Float16 *)(ws + c.samp16);
    float *sampn = (float *)(ws + c.sampn), *sampD = (float *)(ws + c.sampD);
    float *tlo = (float *)(ws + c.tlo), *thi = (float *)(ws + c.thi), *eps = (float *)(ws + c.eps);
    unsigned *cnt_lo = (unsigned *)(ws + c.cnt_lo), *cnt_hi = (unsigned *)(ws + c.cnt_hi);
    float *gstat = (float *)(ws + c.gstat);
    const int ns = (int)((n + RR2_SAMPLE_STRIDE - 1) / RR2_SAMPLE_STRIDE);
    hipLaunchKernelGGL(rr2_norm_stats_kernel, dim3(1), dim3(1024), 0, stream, sqn, n, gstat);
    hipLaunchKernelGGL(rr2_cast_rows_kernel, dim3((unsigned)(c.Np + c.slack)), dim3(256), 0, stream, feat, sqn, n, d, 1, feat16,
                       c.dp, (float *)nullptr);
    hipLaunchKernelGGL(rr2_cast_rows_kernel, dim3((unsigned)c.Nsp), dim3(256), 0, stream, feat, sqn, n, d, RR2_SAMPLE_STRIDE,
                       samp16, c.dp, sampn);
    LAUNCH_CHECK();
    int rc;
    {   // sample pass: [Mp] x [Nsp] one-pass fp16 distances, stored
        GemmArgs a{};
        a.A = feat16 + (size_t)r_lo * c.dp; a.W = samp16; a.M = (int)c.Mp; a.N = (int)c.Nsp; a.K = c.dp;
        a.out = sampD; a.ldo = c.Nsp; a.aux = sqn + r_lo; a.aux2 = sampn; a.m_valid = (int)rows; a.n_valid = ns;
        if ((rc = launch_gemm_f16(a, GE_EUCLID, stream))) return rc;
    }
    hipLaunchKernelGGL(rr2_threshold_kernel, dim3((unsigned)c.Mp), dim3(256), 0, stream, sampD, c.Nsp, ns, rows, RR2_RSEL,
                       sqn + r_lo, gstat, d, tlo, thi, eps, cnt_lo, cnt_hi);
    LAUNCH_CHECK();
    {   // fused pass on the matrix cores, candidates only
        GemmArgs a{};
        a.A = feat16 + (size_t)r_lo * c.dp; a.W = feat16; a.M = (int)c.Mp; a.N = (int)c.Np; a.K = c.dp;
        a.aux = sqn + r_lo; a.aux2 = sqn; a.m_valid = (int)rows; a.n_valid = (int)n;
        a.tlo = tlo; a.thi = thi; a.cnt_lo = cnt_lo; a.cnt_hi = cnt_hi;
        a.list_lo = (uint2 *)(ws + c.list_lo); a.list_hi = (uint2 *)(ws + c.list_hi);
        a.cap_lo = RR2_CAP_LO; a.cap_hi = RR2_CAP_HI; a.sym = sym; a.stagger = stagger;
        if ((rc = launch_gemm_f16(a, GE_CAND, stream))) return rc;
    }
    return MPREID_OK;
}

// Second half: exact refinement of the block's candidate lists, then the rows that could not be certified -- their whole
// distance rows, selected by the dense kernel and scattered back.  rowmax / rank / rankd are indexed by the local row.
int cand_refine(const float *feat, char *ws, const CandBuffers &c, int64_t n, int d, int kr, int64_t r_lo, int64_t rows,
                float *rowmax, int *rank, float *rankd, hipStream_t stream) {
    float *sqn = (float *)(ws + c.sqn);
    unsigned *fb_count = (unsigned *)(ws + c.fb_count);
    int *fb_rows = (int *)(ws + c.fb_rows), *fb_rank = (int *)(ws + c.fb_rank);
    float *fb_feat = (float *)(ws + c.fb_feat), *fb_sqn = (float *)(ws + c.fb_sqn), *fb_D = (float *)(ws + c.fb_D),
          *fb_rowmax = (float *)(ws + c.fb_rowmax);
    const size_t lds = 512 * 8 + RR2_MAXE * 8 + RR2_MAXH * 8 + (size_t)((d + 3) & ~3) * 4 + 2 * 64 * WXD_STRIDE * 4;
    int rc = mpreid_dyn_lds(rr2_refine_kernel<RR2_CAP_LO, RR2_CAP_HI>, lds);
    if (rc) return rc;
    hipLaunchKernelGGL((rr2_refine_kernel<RR2_CAP_LO, RR2_CAP_HI>), dim3((unsigned)rows), dim3(256), lds, stream, feat, sqn, n, d,
                       kr, (unsigned *)(ws + c.cnt_lo), (uint2 *)(ws + c.list_lo), (unsigned *)(ws + c.cnt_hi),
                       (uint2 *)(ws + c.list_hi), (float *)(ws + c.tlo), (float *)(ws + c.eps), rowmax, rank, rankd, fb_count,
                       fb_rows, (unsigned)c.fb_max, r_lo);
    hipLaunchKernelGGL(rr2_fb_gather_kernel, dim3((unsigned)c.fb_max), dim3(256), 0, stream, feat, sqn, d, fb_rows, fb_count,
                       (unsigned)c.fb_max, fb_feat, fb_sqn, r_lo);
    LAUNCH_CHECK();
    if ((rc = mpreid_distance_launch(fb_feat, feat, c.fb_max, n, d, fb_sqn, sqn, fb_D, c.ld, 0, stream, fb_count))) return rc;
    if ((rc = launch_rowmax_topk(fb_D, c.ld, n, kr, c.fb_max, fb_rowmax, fb_rank, stream, fb_count))) return rc;
    hipLaunchKernelGGL(rr2_fb_scatter_kernel, dim3((unsigned)c.fb_max), dim3(256), 0, stream, fb_rows, fb_count,
                       (unsigned)c.fb_max, fb_rowmax, fb_rank, kr, fb_D, c.ld, rowmax, rank, rankd);
    LAUNCH_CHECK();
    return MPREID_OK;
}

// A second HIP stream (per device, created once) for work that is independent of the main chain: the exact distance
// rows of the queries depend only on the features, so the fp32 matrix pipe computes them while the candidate
// refinement / expansion / inverted-index kernels (gathers, LDS, no MFMA) run on the caller's stream.  Fork and join
// with events; to the caller the call is still ordered on `stream`.
struct SideStream {
    hipStream_t s = nullptr;
    hipEvent_t fork = nullptr, join = nullptr, t0 = nullptr, t1 = nullptr;
    int dev = 0;
};
// Side streams are LEASED per call from a per-device pool (created on demand, returned at the end of the call), so that
// calls on different streams / devices of one process never share one and need no process-wide lock.  The lease's
// destructor runs on EVERY exit path: when work was forked onto the side stream it waits for that work first, so the
// workspace (the distance rows it writes) is quiescent when the call returns -- also on the early MPREID_ERR_RETRY_DENSE
// / error returns, after which the caller typically frees or re-purposes the workspace.
struct SideLease {
    SideStream *ss = nullptr;
    bool forked = false;
    static std::mutex &mu() {
        static std::mutex m;
        return m;
    }
    static std::vector<SideStream *> &pool() {
        static std::vector<SideStream *> p;
        return p;
    }
    int acquire() {
        if (ss) return MPREID_OK;
        int dev = 0;
        HIP_TRY(hipGetDevice(&dev));
        {
            std::lock_guard<std::mutex> lk(mu());
            auto &p = pool();
            for (size_t i = 0; i < p.size(); ++i)
                if (p[i]->dev == dev) {
                    ss = p[i];
                    p.erase(p.begin() + (long)i);
                    return MPREID_OK;
                }
        }
        SideStream *n = new SideStream();
        n->dev = dev;
        if (hipStreamCreateWithFlags(&n->s, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&n->fork, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&n->join, hipEventDisableTiming) != hipSuccess || hipEventCreate(&n->t0) != hipSuccess ||
            hipEventCreate(&n->t1) != hipSuccess) {
            mpreid_set_error("re-ranking: could not create the side stream");
            delete n;   // (handles created so far leak on this never-seen path)
            return MPREID_ERR_NODEVICE;
        }
        ss = n;
        return MPREID_OK;
    }
    ~SideLease() {
        if (!ss) return;
        if (forked) (void)hipStreamSynchronize(ss->s);
        std::lock_guard<std::mutex> lk(mu());
        pool().push_back(ss);
    }
};

int rerank_sparse(const float *q, const float *g, int64_t nq, int64_t ng, int d, int k1, int k2, double lambda_value,
                  float *out, int64_t ldo, void *ws, size_t ws_bytes, mpreid_stream_t stream_, mpreid_rerank_stats *stats,
                  int timing, bool split3_rows) {
    ARG_CHECK(q && g && out && nq > 0 && ng > 0 && d > 0 && k1 >= 0 && k2 >= 1 && ldo >= ng);
    const Rerank2Layout L = make_layout2(nq, ng, d, k1, k2, split3_rows);
    const int64_t N = L.N;
    if (N >= (1ll << 28) - 512) {
        mpreid_set_error("N too large for the sparse algorithm");
        return MPREID_ERR_UNSUPPORTED;
    }
    if (!ws || ws_bytes < L.total) {
        mpreid_set_error("rerank workspace too small: %zu < %zu", ws_bytes, L.total);
        return MPREID_ERR_WORKSPACE;
    }
    hipStream_t stream = (hipStream_t)stream_;
    SideLease lease;   // (declared before anything that can return: its destructor joins the side stream on every path)
    char *base = (char *)ws;
    float *feat = (float *)(base + L.feat), *sqn = (float *)(base + L.c.sqn), *gstat = (float *)(base + L.c.gstat);
    float *rowmax = (float *)(base + L.rowmax), *rankd = (float *)(base + L.rankd);
    int *rank = (int *)(base + L.rank);
    unsigned *fb_count = (unsigned *)(base + L.c.fb_count);
    int *vcnt = (int *)(base + L.vcnt), *vidx = (int *)(base + L.vidx);
    uint16_t *vval = (uint16_t *)(base + L.vval);
    int *ucnt = (int *)(base + L.ucnt);
    float *dq = (float *)(base + L.dq);
    unsigned long long *counters = (unsigned long long *)(base + L.counters);

    StageTimer tm(timing != 0, stream);
    HIP_TRY(hipMemsetAsync(counters, 0, 64, stream));
    HIP_TRY(hipMemsetAsync(fb_count, 0, 64, stream));
    // rows that need the fallback but do not fit its buffer keep these values: the call then ends with
    // MPREID_ERR_RETRY_DENSE, but every kernel on the way must still see valid neighbour indices
    HIP_TRY(hipMemsetAsync(rank, 0, (size_t)N * L.KR * 4, stream));
    HIP_TRY(hipMemsetAsync(rankd, 0, (size_t)N * L.KR * 4, stream));
    HIP_TRY(hipMemsetAsync(rowmax, 0, (size_t)N * 4, stream));
    tm.mark(); // 0
    // features, exact squared norms (padded with zeros), fp16 operands, sample
    HIP_TRY(hipMemcpyAsync(feat, q, (size_t)nq * d * 4, hipMemcpyDeviceToDevice, stream));
    HIP_TRY(hipMemcpyAsync(feat + (size_t)nq * d, g, (size_t)ng * d * 4, hipMemcpyDeviceToDevice, stream));
    HIP_TRY(hipMemsetAsync(sqn, 0, (size_t)L.c.Np * 4, stream));
    int rc = mpreid_sqnorm_f32(feat, N, d, sqn, stream);
    if (rc) return rc;
    static const int cand_dbg = mpreid_ablation_env("MPREID_CAND_DBG");   // timing experiments (wrong results)
    rc = cand_lists(feat, base, L.c, N, d, 0, N, (cand_dbg & 1) ? 0 : 1, (cand_dbg & 2) ? 2 : 0, stream);
    if (rc) return rc;
    tm.mark(); // 1
    // exact distance rows of the queries (what the Jaccard blend reads): only the GALLERY columns [nq, N) of the query rows are ever read (the blend of final_dist[:nq, nq:]): the first
    // nq columns of dq stay unwritten (20 % of the fp32 matrix work at nq = N / 5)
    auto launch_dq = [&](hipStream_t s, int64_t q0, int64_t rows) -> int {
        if (N == nq || rows <= 0) return MPREID_OK;
        // MPREID_RERANK_SPARSE_SPLIT3: the rows that only feed the blend term lambda * d / max come from the fp16 matrix
        // cores (3-term split, |error| <= 1e-6: |delta final| <= lambda * 1e-6 / max); everything discrete -- neighbours,
        // V, V_qe, the Jaccard term -- is computed exactly as in the bit-parity mode
        if (split3_rows)
            return mpreid_distance_f16_split3(feat + (size_t)q0 * d, feat + (size_t)nq * d, rows, N - nq, d, sqn + q0, sqn + nq,
                                              dq + (size_t)q0 * L.ld + nq, L.ld, 0, base + L.dq_ws, L.dq_ws_bytes, s);
        return mpreid_distance_launch(feat + (size_t)q0 * d, feat + (size_t)nq * d, rows, N - nq, d, sqn + q0, sqn + nq,
                                      dq + (size_t)q0 * L.ld + nq, L.ld, 0, s);
    };
    // Overlap of the fp32 matrix work with the rest (MPREID_TUNE rerank_overlap = 0 / 1 forces it off / on): one launch on
    // the side stream, forked AFTER the fused GEMM (a persistent kernel that owns every CU's LDS: forked before it, the
    // two GEMMs only take turns).  Nearly zero-sum wherever it was measured: N = 20 000 6.06 vs 6.04 ms, N = 100 000
    // 87.7 -> 86.2 ms, MSMT17 shape 77.7 -> 76.7 ms (on by default only from N = 50 000).  Also measured at N = 100 000
    // and NOT kept: the rows in four query blocks forked after the V rows so that the Jaccard stage of block b runs
    // beside the rows of block b + 1 -- 87.0 ms as launched (the GEMM's workgroups take every slot that frees up and
    // the partner starves), 90.2 ms against 90.7 in line with the GEMM made persistent at two workgroups per CU so that
    // both kernels are resident (both then run at half speed: they share each CU's load path and LDS).
    static const int ov_tune = mpreid_tune("rerank_overlap", -1);
    const int ov_mode = ov_tune >= 0 ? (ov_tune != 0) : (N < 50000 ? 0 : 1);
    const bool no_overlap = ov_mode == 0;
    SideStream *ss = nullptr;
    if (ov_mode != 0) {
        if ((rc = lease.acquire())) return rc;
        ss = lease.ss;
    }
    if (ov_mode == 1) {
        HIP_TRY(hipEventRecord(ss->fork, stream));
        HIP_TRY(hipStreamWaitEvent(ss->s, ss->fork, 0));
        lease.forked = true;
        if (timing) HIP_TRY(hipEventRecord(ss->t0, ss->s));
        if ((rc = launch_dq(ss->s, 0, nq))) return rc;
        if (timing) HIP_TRY(hipEventRecord(ss->t1, ss->s));
        HIP_TRY(hipEventRecord(ss->join, ss->s));
    }
    rc = cand_refine(feat, base, L.c, N, d, L.KR, 0, N, rowmax, rank, rankd, stream);   // refinement + fallback rows
    if (rc) return rc;
    launch_sum_i32((const int *)(base + L.c.cnt_lo), N, counters + 5, stream);
    HIP_TRY(hipMemcpyAsync(counters + 4, fb_count, 4, hipMemcpyDeviceToDevice, stream));
    LAUNCH_CHECK();
    tm.mark(); // 2
    {   // V rows, distances on the fly
        rc = launch_krecip(true, nullptr, L.ld, N, rowmax, rank, L.K, L.KR, L.h, L.vcap, vcnt, vidx, vval, 0, N, ucnt, feat, sqn, d,
                           rankd, (unsigned *)(base + L.rbits), stream);
        if (rc) return rc;
        launch_sum_i32(ucnt, N, counters + 1, stream);
        LAUNCH_CHECK();
    }
    tm.mark(); // 3
    TailArgs ta{};
    SideStream *evs = nullptr;
    if (no_overlap) {   // exact distance rows of the queries, in line: launched by the tail (see TailArgs::mid_launch)
        if ((rc = lease.acquire())) return rc;     // (only its `fork` event is used here)
        evs = lease.ss;
        ta.mid_launch = [&](hipStream_t s) -> int { return launch_dq(s, 0, nq); };
        ta.sized = evs->fork;
    }
    ta.N = N; ta.nq = nq; ta.k1 = k1; ta.k2 = k2; ta.KR = L.KR; ta.h = L.h; ta.vcap = L.vcap; ta.qcap_bound = L.qcap_bound;
    ta.rank = rank; ta.vcnt = vcnt; ta.vidx = vidx; ta.vval = vval; ta.ucnt = ucnt; ta.qcnt = (int *)(base + L.qcnt);
    ta.qidx = (int *)(base + L.qidx); ta.qval = (uint16_t *)(base + L.qval); ta.ccnt = (unsigned *)(base + L.ccnt);
    ta.cptr = (long long *)(base + L.cptr); ta.crow = (int *)(base + L.crow); ta.cval = (uint16_t *)(base + L.cval);
    ta.chist = (unsigned *)(base + L.chist);
    ta.counters = counters; ta.MT = dq; ta.ld = L.ld; ta.rowmax = rowmax; ta.out = out; ta.ldo = ldo;
    ta.lambda_value = lambda_value; ta.algo = split3_rows ? MPREID_RERANK_SPARSE_SPLIT3 : MPREID_RERANK_SPARSE;
    ta.join = ss ? ss->join : nullptr;
    rc = rerank_tail(ta, stream, tm, stats, 3);
    if (rc) return rc;
    if (ss && timing && stats) {   // the side stream's own duration (it overlaps the main chain)
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ss->t0, ss->t1) == hipSuccess) stats->ms_dq = ms;
    }
    // status of the data-dependent capacities (read with the statistics, after the fact): the fp16 operands must
    // not have overflowed and the fallback rows must have fitted their buffer -- otherwise the result above is not
    // valid and the caller repeats the call with the dense algorithm
    float gs[2] = {0.f, 0.f};
    unsigned fbc = 0;
    HIP_TRY(hipMemcpy(gs, gstat, 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&fbc, fb_count, 4, hipMemcpyDeviceToHost));
    if (gs[1] != 0.0f || fbc > (unsigned)L.c.fb_max) {
        mpreid_set_error("sparse re-ranking: %s; retry with MPREID_RERANK_DENSE",
                         gs[1] != 0.0f ? "row norms too large for fp16 operands" : "too many rows needed the dense fallback");
        return MPREID_ERR_RETRY_DENSE;
    }
    return MPREID_OK;
}
