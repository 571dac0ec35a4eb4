// ---------------------------------------------------------------------------------------------
// rerank_wide.hip — the WIDE algorithm: its workspace layout, its five kernels, its driver.
// WIDE algorithm: any k1 / k2 (utils/reranking.py:29 takes any; DENSE / SPARSE stop at max(k1 + 1, k2) = 256 and at the
// LDS a row's expansion lists need).  A completeness path: the same arithmetic and the same bits as DENSE, with every
// table whose size grows with k moved from LDS into the workspace.  What stays in LDS is a function of N alone (two N-bit
// masks, 2 * N / 8 bytes: 160 KiB at N = 655 360, where the N x N fp32 matrix of the workspace would be 1.7 TB) or a
// constant.  Reused as they are: the exact distance GEMM, make_mt_kernel, csc_count / csc_scan / csc_fill (row stride and
// offsets are 64-bit there), sum_i32_kernel.  New: the five kernels below.
//
// Kernels that need per-row scratch run a capped grid (wide_wg_count workgroups) that strides over the rows, so the scratch
// is per WORKGROUP ([wg][P] sort keys, [wg][vcap] weights, [wg][N] accumulators: L2-resident) and not per row.
// ---------------------------------------------------------------------------------------------
#include "rerank.h"

constexpr int WIDE_WG_MAX = 1024;          // 256 CUs x 4 workgroups of 256 threads
WideLayout make_layout_wide(int64_t nq, int64_t ng, int d, int k1, int k2, int has_local) {
    static const int sort_lds = mpreid_tune("wide_sort_lds", 4096);       // largest sort that runs in LDS (keys of 8 bytes)
    static const int jrows = mpreid_tune("wide_jaccard_rows", 24576);     // fp16 accumulators of one Jaccard chunk (48 KB)
    WideLayout L{};
    L.N = nq + ng;
    L.ld = (int64_t)align_up((size_t)L.N, 64);
    static_cast<RerankK &>(L) = clamp_k(L.N, k1, k2);   // the clamped k's: one definition for all algorithms
    L.qcap = (k2 != 1) ? L.qcap_bound : 0;            // V_qe rows are sized for the bound (no sizing pass, no host round trip)
    L.fcap = (k2 != 1) ? (int)L.qcap : L.vcap;        // row stride of the matrix the inverted index is built from
    L.P = 1;
    while (L.P < L.KR) L.P <<= 1;                     // bitonic network size of the neighbour sort
    L.sort_in_lds = L.P <= std::max(1, std::min(sort_lds, 8192));
    L.nwg = (int)std::max<int64_t>(1, std::min<int64_t>(L.N, WIDE_WG_MAX));
    L.rch = (int)align_up((size_t)std::max<int64_t>(1, std::min<int64_t>(ng, std::max(8, std::min(jrows, 65536)))), 8);
    WsCursor take;
    const size_t N = (size_t)L.N, M = (size_t)ng;
    L.feat = take(N * (size_t)d * 4);
    L.norms = take(N * 4);
    L.D = take(N * (size_t)L.ld * 4);
    L.MT = has_local ? take(N * (size_t)L.ld * 4) : L.D;
    L.rowmax = take(N * 4);
    L.rank = take(N * (size_t)L.KR * 4);
    L.rsort = take(N * (size_t)L.K * 8);
    L.rpos = take(N * (size_t)L.K * 4);
    L.sortscr = take(L.sort_in_lds ? 0 : (size_t)L.nwg * (size_t)L.P * 8);
    L.rcount = take(N * 4);
    L.vcnt = take(N * 4);
    L.vidx = take(N * (size_t)L.vcap * 4);
    L.vval = take(N * (size_t)L.vcap * 2);
    L.wscr = take((size_t)L.nwg * (size_t)L.vcap * 4);
    L.qcnt = take(N * 4);
    L.qidx = take(N * (size_t)L.qcap * 4);
    L.qval = take(N * (size_t)L.qcap * 2);
    L.accscr = take(k2 != 1 ? (size_t)L.nwg * N * 4 : 0);
    L.ccnt = take((N + 1) * 4);
    L.cptr = take((N + 1) * 8);
    L.crow = take(M * (size_t)L.fcap * 4);            // the inverted index holds the gallery rows only
    L.cval = take(M * (size_t)L.fcap * 2);
    L.counters = take(64);
    L.total = take.off;
    return L;
}

// ascending bitonic sort of buf[0..P) (P a power of two; LDS or global memory), 256 threads.  Ends with a barrier.
__device__ __forceinline__ void wide_bitonic_sort(unsigned long long *buf, int P, int tid) {
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < (P >> 1); t += 256) {
                const int lo = ((t & ~(stride - 1)) << 1) | (t & (stride - 1));
                const int hi = lo + stride;
                const unsigned long long a = buf[lo], b = buf[hi];
                const bool up = ((lo & size) == 0);
                if ((a > b) == up) {
                    buf[lo] = b;
                    buf[hi] = a;
                }
            }
            __syncthreads();
        }
    }
}

// (2)+(3) row max and the first KR entries of the row in ascending (O value, index) order, any KR <= N.
// The threshold search is the radix-histogram search of rowmax_topk_kernel (11 + 11 + 10 bits, the row re-read from L2 per
// pass); the winners go to a P-entry key array (LDS up to wide_sort_lds entries, else this workgroup's slice of the
// workspace) and are ordered by a multi-pass bitonic network over all P = pow2(KR) entries -- KR = N is a full row sort.
// Also written: rsort[i][0..K) = (index << 32 | position) of the first K neighbours ordered by INDEX, the table the
// reciprocity tests search (wide_recip_kernel).
__global__ __launch_bounds__(256) void wide_topk_kernel(const float *__restrict__ MT, int64_t ld, int64_t N, int K, int KR, int P,
                                                        float *__restrict__ rowmax, int *__restrict__ rank,
                                                        unsigned long long *__restrict__ rsort,
                                                        unsigned long long *__restrict__ sortscr) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ unsigned hist[2048];
    __shared__ float s_red[4];
    __shared__ int s_wave[4];
    __shared__ unsigned s_bin, s_below, s_cnt;
    unsigned long long *buf = sortscr ? sortscr + (size_t)blockIdx.x * (size_t)P : (unsigned long long *)smem;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = (int)N;
    int PK = 1;
    while (PK < K) PK <<= 1;
    for (int64_t i = blockIdx.x; i < N; i += gridDim.x) {
        const float *row = MT + i * ld;
        float mx = -3.402823466e+38f;
        for (int j = tid; j < n; j += 256) mx = fmaxf(mx, row[j]);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
        __syncthreads();   // (the previous row's readers of s_red / buf are done)
        if (lane == 0) s_red[wave] = mx;
        __syncthreads();
        mx = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
        if (tid == 0) rowmax[i] = mx;

        // exact key T of the KR-th smallest entry; kk of the cnt_eq entries equal to T are taken
        unsigned prefix = 0;
        int kk = KR, bits_done = 0;
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
            }
            __syncthreads();
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
        const unsigned T = prefix;

        for (int t = tid; t < P; t += 256) buf[t] = ~0ull;
        if (tid == 0) s_cnt = 0;
        __syncthreads();
        if ((int)cnt_eq == kk) {
            // no tie straddles the cut: exactly KR keys are <= T; their order is fixed by the sort
            for (int j = tid; j < n; j += 256) {
                const unsigned key = fkey(__fdiv_rn(row[j], mx));
                if (key <= T) {
                    const unsigned p = atomicAdd(&s_cnt, 1u);
                    if (p < (unsigned)KR) buf[p] = ((unsigned long long)key << 32) | (unsigned)j;
                }
            }
        } else {
            // ties at the cut: the kk smallest INDICES among the equal keys (ordered scans)
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
                if (accept && p < KR) buf[p] = ((unsigned long long)key << 32) | (unsigned)j;
                run_acc += acc_tot;
                run_eq += eq_tot;
            }
        }
        __syncthreads();
        wide_bitonic_sort(buf, P, tid);
        // rank row; then the same entries keyed (index, position) for the first K, sorted again (every thread rewrites the
        // slots it read itself)
        for (int t = tid; t < P; t += 256) {
            const unsigned idx = (unsigned)(buf[t] & 0xffffffffull);
            if (t < KR) rank[i * KR + t] = (int)idx;
            buf[t] = (t < K) ? (((unsigned long long)idx << 32) | (unsigned)t) : ~0ull;
        }
        __syncthreads();
        wide_bitonic_sort(buf, PK, tid);
        for (int t = tid; t < K; t += 256) rsort[i * K + t] = buf[t];
    }
}

// Reciprocity of the neighbour table, once per row (recip_bits_kernel without the 256-bit masks): for row c and position
// a < K with n = rank[c][a],  rpos[c][a] = position of c in rank[n][0..K)  or -1.
//   n is a k-reciprocal neighbour of c      <=>  rpos[c][a] >= 0                      (utils/reranking.py:53-58)
//   n is a k1/2-reciprocal neighbour of c   <=>  a < h and 0 <= rpos[c][a] < h        (:61-66)
// Found by binary search in the index-sorted copy rsort[n] (8-byte entries): N * K * ceil(log2 K) loads of 8 bytes, 9 per
// pair at K = 300 (21 MB per 1000 rows, L2 hits for the first levels) -- chosen over N-bit masks per row (N * N / 8 bytes
// of workspace and a full-row scatter per row) and over the linear scan of the table (N * K * K * 4 bytes of traffic).
__global__ __launch_bounds__(256) void wide_recip_kernel(const int *__restrict__ rank, const unsigned long long *__restrict__ rsort,
                                                         int64_t N, int K, int KR, int *__restrict__ rpos) {
    const int lane = threadIdx.x & 63;
    const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= N) return;
    for (int a = lane; a < K; a += 64) {
        const int64_t n = rank[c * KR + a];
        const unsigned long long *srt = rsort + n * K;
        int lo = 0, hi = K;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((unsigned)(srt[mid] >> 32) < (unsigned)c) lo = mid + 1; else hi = mid;
        }
        int p = -1;
        if (lo < K) {
            const unsigned long long e = srt[lo];
            if ((unsigned)(e >> 32) == (unsigned)c) p = (int)(unsigned)(e & 0xffffffffull);
        }
        rpos[c * K + a] = p;
    }
}

// (4)-(6) k-reciprocal set, 2/3-overlap expansion, exp weights, V row (utils/reranking.py:51-71); the arithmetic of
// krecip_kernel with the lists in the workspace.  LDS: two N-bit masks (R and the expansion set).  One wave per candidate
// of the expansion; the sorted expansion list is extracted straight into the row's vidx slots, the weights go to this
// workgroup's scratch, wave 0 runs the numpy-order pairwise sum and compacts the row in place (write position <= read
// position, one wave, 64 entries read before any of them is written).
__global__ __launch_bounds__(256) void wide_krecip_kernel(const float *__restrict__ MT, int64_t ld, int64_t N,
                                                          const float *__restrict__ rowmax, const int *__restrict__ rank,
                                                          const int *__restrict__ rpos, int K, int KR, int h, int vcap,
                                                          int *__restrict__ vcnt, int *vidx, uint16_t *__restrict__ vval,
                                                          float *wscr, int *__restrict__ r_count) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int nw = (int)((N + 31) >> 5);
    unsigned *Rmask = (unsigned *)smem, *Emask = Rmask + nw;
    __shared__ int s_nR, s_nE;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float *wbuf = wscr + (size_t)blockIdx.x * (size_t)vcap;
    for (int64_t i = blockIdx.x; i < N; i += gridDim.x) {
        for (int w = tid; w < nw; w += 256) {
            Rmask[w] = 0u;
            Emask[w] = 0u;
        }
        if (tid == 0) s_nR = 0;
        __syncthreads();
        const int *fwd = rank + i * KR;
        const int *fpos = rpos + i * K;
        for (int a = tid; a < K; a += 256) {
            if (fpos[a] >= 0) {
                const int c = fwd[a];
                atomicOr(&Rmask[c >> 5], 1u << (c & 31));
                atomicOr(&Emask[c >> 5], 1u << (c & 31));
                atomicAdd(&s_nR, 1);
            }
        }
        __syncthreads();
        for (int a = wave; a < K; a += 4) {   // wave-uniform
            if (fpos[a] < 0) continue;
            const int64_t cand = fwd[a];
            const int *cf = rank + cand * KR;
            const int *cp = rpos + cand * K;
            int nRc = 0, inter = 0;
            for (int b0 = 0; b0 < h; b0 += 64) {
                const int b = b0 + lane;
                bool ok = false, inr = false;
                if (b < h) {
                    const int p = cp[b];
                    ok = p >= 0 && p < h;
                    if (ok) {
                        const int f = cf[b];
                        inr = (Rmask[f >> 5] >> (f & 31)) & 1u;
                    }
                }
                nRc += __popcll(__ballot(ok));
                inter += __popcll(__ballot(inr));
            }
            if ((double)inter > (2.0 / 3.0) * (double)nRc) {
                for (int b = lane; b < h; b += 64) {
                    const int p = cp[b];
                    if (p >= 0 && p < h) {
                        const int f = cf[b];
                        atomicOr(&Emask[f >> 5], 1u << (f & 31));
                    }
                }
            }
        }
        __syncthreads();
        int *Elist = vidx + i * vcap;   // np.unique(expansion index): the set bits in ascending order
        if (wave == 0) {
            const int ne = extract_bits_sorted(Emask, nw, Elist, lane);
            if (lane == 0) s_nE = ne;
        }
        __syncthreads();
        const int nE = s_nE;
        const float mx = rowmax[i];
        const float *row = MT + i * ld;
        for (int t = tid; t < nE; t += 256) wbuf[t] = mpreid_np_expf(-__fdiv_rn(row[Elist[t]], mx));
        __syncthreads();
        if (wave == 0) {
            const float s = wave_pairwise_sum(wbuf, nE, lane);
            int out = 0;
            for (int t0 = 0; t0 < nE; t0 += 64) {
                const int t = t0 + lane;
                uint16_t hv = 0;
                int e = 0;
                if (t < nE) {
                    e = Elist[t];
                    hv = h_from_f32(__fdiv_rn(wbuf[t], s));
                }
                const bool nz = (hv & 0x7fffu) != 0;
                const unsigned long long m = __ballot(nz);
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");   // the 64 reads of Elist precede the writes below
                if (nz) {
                    const int p = out + __popcll(m & ((1ull << lane) - 1ull));
                    Elist[p] = e;
                    vval[i * vcap + p] = hv;
                }
                out += __popcll(m);
            }
            if (lane == 0) {
                vcnt[i] = out;
                r_count[i] = s_nR;
            }
        }
        __syncthreads();
    }
}

// (7) local query expansion (utils/reranking.py:73-78) with a dense fp32 accumulator row [N] per workgroup in the workspace
// instead of acc[qcap] / ulist[qcap] in LDS: the k2 neighbour rows are added one after the other (rank order, a barrier
// between two rows; the entries of one row are distinct columns), then the row is divided by fp32(k2), rounded to fp16 and
// compacted in ascending column order.  V entries are positive, so a touched column has a non-zero sum and an untouched one
// rounds to the zero the compaction drops anyway -- no union mask is needed.
__global__ __launch_bounds__(256) void wide_qe_kernel(int64_t N, const int *__restrict__ rank, int KR, int k2,
                                                      const int *__restrict__ vcnt, const int *__restrict__ vidx,
                                                      const uint16_t *__restrict__ vval, int vcap, int64_t qcap,
                                                      int *__restrict__ qcnt, int *__restrict__ qidx,
                                                      uint16_t *__restrict__ qval, float *accscr) {
    __shared__ int s_wave[4];
    const int tid = threadIdx.x;
    float *acc = accscr + (size_t)blockIdx.x * (size_t)N;
    const float k2f = (float)k2;
    for (int64_t i = blockIdx.x; i < N; i += gridDim.x) {
        for (int64_t c = tid; c < N; c += 256) acc[c] = 0.0f;
        __syncthreads();
        for (int m = 0; m < k2; ++m) {
            const int64_t r = rank[i * KR + m];
            const int cnt = vcnt[r];
            for (int a = tid; a < cnt; a += 256) {
                const int c = vidx[r * vcap + a];
                acc[c] = acc[c] + h_to_f32(vval[r * vcap + a]);
            }
            __syncthreads();
        }
        int run = 0;
        for (int64_t c0 = 0; c0 < N; c0 += 256) {
            const int64_t c = c0 + tid;
            uint16_t hv = 0;
            if (c < N) hv = h_from_f32(__fdiv_rn(acc[c], k2f));
            const bool nz = (hv & 0x7fffu) != 0;
            int tot;
            const int p = run + block_excl_scan_256(nz ? 1 : 0, tid, s_wave, tot);
            if (nz && (int64_t)p < qcap) {
                qidx[i * qcap + p] = (int)c;
                qval[i * qcap + p] = hv;
            }
            run += tot;
        }
        if (tid == 0) qcnt[i] = run;
        __syncthreads();
    }
}

// (8)-(11) Jaccard min-sum + blend (utils/reranking.py:84-100) without per-query tables in LDS: the query's own row
// (column index, value) and the column bounds are read from the workspace as the columns are walked (the next column's
// four words are requested before the current column is applied); LDS holds the fp16 accumulators of one chunk of rch
// gallery rows only.  Sequential fp16 accumulation in ascending column order: the rows of a column are distinct, one
// barrier separates two columns.  With more than one chunk (ng > rch) every workgroup walks whole columns and keeps
// the rows of its chunk: nchunks x the gather traffic, the price of needing no blocked index.
__global__ __launch_bounds__(256) void wide_jaccard_kernel(int64_t N, int64_t nq, const float *__restrict__ MT, int64_t ld,
                                                           const float *__restrict__ rowmax, const int *__restrict__ fcnt,
                                                           const int *__restrict__ fidx, const uint16_t *__restrict__ fval,
                                                           int64_t fcap, const long long *__restrict__ cptr,
                                                           const int *__restrict__ crow, const uint16_t *__restrict__ cval,
                                                           int rch, uint16_t one_minus_lam_h, float lam32,
                                                           float *__restrict__ out, int64_t ldo,
                                                           unsigned long long *__restrict__ pair_counter) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint16_t *t = (uint16_t *)smem;   // [rch]
    const int tid = threadIdx.x;
    const int64_t i = blockIdx.x;
    const int64_t r0 = nq + (int64_t)blockIdx.y * rch;
    const int64_t r1 = (r0 + rch < N) ? r0 + rch : N;
    const int cnt = fcnt[i];
    const int *qi = fidx + i * fcap;
    const uint16_t *qv = fval + i * fcap;
    for (int r = tid; r < rch; r += 256) t[r] = 0;
    __syncthreads();
    unsigned long long pairs = 0;
    int c_nx = 0;
    uint16_t v_nx = 0;
    long long p0_nx = 0, p1_nx = 0;
    if (cnt > 0) {
        c_nx = qi[0];
        v_nx = qv[0];
        p0_nx = cptr[c_nx];
        p1_nx = cptr[c_nx + 1];
    }
    for (int a = 0; a < cnt; ++a) {
        const uint16_t vic = v_nx;
        const long long p0 = p0_nx, p1 = p1_nx;
        if (a + 1 < cnt) {
            c_nx = qi[a + 1];
            v_nx = qv[a + 1];
            p0_nx = cptr[c_nx];
            p1_nx = cptr[c_nx + 1];
        }
        pairs += (unsigned long long)(p1 - p0);
        for (long long p = p0 + tid; p < p1; p += 256) {
            const int64_t r = crow[p];
            if (r >= r0 && r < r1) t[r - r0] = h_add_native(t[r - r0], mpreid_h_min_nonneg(vic, cval[p]));
        }
        __syncthreads();
    }
    if (pair_counter && tid == 0 && blockIdx.y == 0 && pairs) atomicAdd(pair_counter, pairs);
    const float mx = rowmax[i];
    const float *row = MT + i * ld;
    const uint16_t H1 = 0x3c00u, H2 = 0x4000u;
    for (int64_t j = r0 + tid; j < r1; j += 256) {
        const uint16_t tv = t[j - r0];
        const uint16_t den = h_sub_native(H2, tv);
        const uint16_t qt = h_div_native(tv, den);
        const uint16_t jac = h_sub_native(H1, qt);
        const uint16_t jl = h_mul_native(jac, one_minus_lam_h);
        const float o = __fdiv_rn(row[j], mx);
        out[i * ldo + (j - nq)] = h_to_f32(jl) + o * lam32;
    }
}

// the only refusals of WIDE: N, and the two N-bit masks of wide_krecip_kernel (never binding before the workspace is)
bool wide_fits(int64_t nq, int64_t ng) {
    const int64_t N = nq + ng;
    return N >= 1 && N < (1ll << 31) - 64 && (size_t)((N + 31) >> 5) * 8 <= LDS_WG_MAX;
}

int rerank_wide(const float *q, const float *g, int64_t nq, int64_t ng, int d, int k1, int k2, double lambda_value,
                const float *local, int only_local, float *out, int64_t ldo, void *ws, size_t ws_bytes,
                mpreid_stream_t stream_, mpreid_rerank_stats *stats, int timing) {
    ARG_CHECK(q && g && out && nq > 0 && ng > 0 && d > 0 && k1 >= 0 && k2 >= 1 && ldo >= ng);
    ARG_CHECK(!only_local || local);
    if (!wide_fits(nq, ng)) {
        mpreid_set_error("re_ranking (WIDE): N = %lld is too large (N < 2^31 - 64 and N / 4 bytes of LDS masks)", (long long)(nq + ng));
        return MPREID_ERR_UNSUPPORTED;
    }
    const WideLayout L = make_layout_wide(nq, ng, d, k1, k2, local != nullptr);
    const int64_t N = L.N;
    if (!ws || ws_bytes < L.total) {
        mpreid_set_error("rerank workspace too small: %zu < %zu", ws_bytes, L.total);
        return MPREID_ERR_WORKSPACE;
    }
    hipStream_t stream = (hipStream_t)stream_;
    char *base = (char *)ws;
    float *feat = (float *)(base + L.feat), *norms = (float *)(base + L.norms);
    float *D = (float *)(base + L.D), *MT = (float *)(base + L.MT), *rowmax = (float *)(base + L.rowmax);
    int *rank = (int *)(base + L.rank), *rpos = (int *)(base + L.rpos), *rcount = (int *)(base + L.rcount);
    unsigned long long *rsort = (unsigned long long *)(base + L.rsort);
    unsigned long long *sortscr = L.sort_in_lds ? nullptr : (unsigned long long *)(base + L.sortscr);
    int *vcnt = (int *)(base + L.vcnt), *vidx = (int *)(base + L.vidx);
    uint16_t *vval = (uint16_t *)(base + L.vval);
    float *wscr = (float *)(base + L.wscr), *accscr = (float *)(base + L.accscr);
    int *qcnt = (int *)(base + L.qcnt), *qidx = (int *)(base + L.qidx);
    uint16_t *qval = (uint16_t *)(base + L.qval);
    unsigned *ccnt = (unsigned *)(base + L.ccnt);
    long long *cptr = (long long *)(base + L.cptr);
    int *crow = (int *)(base + L.crow);
    uint16_t *cval = (uint16_t *)(base + L.cval);
    unsigned long long *counters = (unsigned long long *)(base + L.counters);
    const int nw = (int)((N + 31) >> 5);
    const int k2e = (int)std::min<int64_t>(k2, N);

    StageTimer tm(timing != 0, stream);
    HIP_TRY(hipMemsetAsync(counters, 0, 64, stream));
    tm.mark(); // 0
    {   // (1) original_dist
        int rc = launch_original_dist(q, g, nq, ng, d, local, only_local, feat, norms, D, MT, L.ld, stream);
        if (rc) return rc;
    }
    tm.mark(); // 1
    // (2)+(3) row max, neighbour table, its index-sorted copy, reciprocity positions
    {
        const size_t lds = L.sort_in_lds ? (size_t)L.P * 8 : 0;
        int rc = mpreid_dyn_lds(wide_topk_kernel, lds);
        if (rc) return rc;
        hipLaunchKernelGGL(wide_topk_kernel, dim3((unsigned)L.nwg), dim3(256), lds, stream, MT, L.ld, N, L.K, L.KR, L.P, rowmax,
                           rank, rsort, sortscr);
        hipLaunchKernelGGL(wide_recip_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, stream, rank, rsort, N, L.K, L.KR, rpos);
        LAUNCH_CHECK();
    }
    tm.mark(); // 2
    // (4)-(6) V rows
    {
        const size_t lds = (size_t)nw * 8;
        int rc = mpreid_dyn_lds(wide_krecip_kernel, lds);
        if (rc) return rc;
        hipLaunchKernelGGL(wide_krecip_kernel, dim3((unsigned)L.nwg), dim3(256), lds, stream, MT, L.ld, N, rowmax, rank, rpos, L.K,
                           L.KR, L.h, L.vcap, vcnt, vidx, vval, wscr, rcount);
        launch_sum_i32(rcount, N, counters + 1, stream);
        launch_sum_i32(vcnt, N, counters + 2, stream);
        LAUNCH_CHECK();
    }
    tm.mark(); // 3
    // (7) query expansion
    const int *fcnt = vcnt, *fidx = vidx;
    const uint16_t *fval = vval;
    if (k2 != 1) {
        hipLaunchKernelGGL(wide_qe_kernel, dim3((unsigned)L.nwg), dim3(256), 0, stream, N, rank, L.KR, k2e, vcnt, vidx, vval, L.vcap,
                           L.qcap, qcnt, qidx, qval, accscr);
        LAUNCH_CHECK();
        fcnt = qcnt;
        fidx = qidx;
        fval = qval;
    }
    launch_sum_i32(fcnt, N, counters + 6, stream);
    tm.mark(); // 4
    // inverted index of the gallery rows (the atomic-cursor build: its row stride and offsets are 64-bit)
    {
        int rc = launch_csc_atomic(N, nq, fcnt, fidx, fval, L.fcap, ccnt, cptr, crow, cval, stream);
        if (rc) return rc;
        LAUNCH_CHECK();
    }
    tm.mark(); // 5
    // (8)-(11) Jaccard + blend
    {
        const size_t lds = align_up((size_t)L.rch * 2, 16);
        int rc = mpreid_dyn_lds(wide_jaccard_kernel, lds);
        if (rc) return rc;
        const unsigned nchunks = (unsigned)((ng + L.rch - 1) / L.rch);
        hipLaunchKernelGGL(wide_jaccard_kernel, dim3((unsigned)nq, nchunks), dim3(256), lds, stream, N, nq, MT, L.ld, rowmax, fcnt,
                           fidx, fval, (int64_t)L.fcap, cptr, crow, cval, L.rch, f64_to_f16_host(1.0 - lambda_value),
                           (float)lambda_value, out, ldo, counters);
        LAUNCH_CHECK();
    }
    tm.mark(); // 6
    unsigned long long cnt[7] = {0, 0, 0, 0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(cnt, counters, sizeof(cnt), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    fill_rerank_stats(stats, N, k1, k2, L.h, L.vcap, L.fcap, cnt, MPREID_RERANK_WIDE, tm, 3, 4, 4, 4, false);
    return MPREID_OK;
}
