// rerank.hip — k-reciprocal re-ranking on gfx950 (reference: utils/reranking.py:29-100): stages (7)-(11) -- query expansion, the
// inverted index of V_qe (blocked counting sort and atomic-cursor build), Jaccard + blend -- with the tail that drives them for the
// dense and the sparse single call, the dense layout and driver, and the public single-call entry points; then the row-sharded C API.  rerank.h has the map.
#include "rerank.h"

JaccardPlan jaccard_plan(int64_t N) {
    constexpr int B = 256;   // = CSC_B
    static const int jwave = mpreid_tune("jaccard_wave", -1);
    static const int jrows = mpreid_tune("jaccard_wave_rows", 10240);
    JaccardPlan p;
    p.rpb = (int)((N + B - 1) / B);
    // 256-thread form: at most ~24 K rows per chunk (48 KB of accumulators: two workgroups per CU beside the tables)
    p.bpc = std::max(1, std::min(B, 24576 / p.rpb));
    p.nchunks = (B + p.bpc - 1) / p.bpc;
    // more than one chunk: ONE wave per (query, chunk of ~10 K rows) -- no barriers at all (the LDS operations of a wave
    // execute in order, which is all the fp16 accumulation order needs), LDS = the accumulators only (jaccard_wave_kernel;
    // measured at N = 100 000 / MSMT17 shape: 4 K rows 15.6 / 10.2 ms, 6 K 14.6 / 8.6, 8 K 14.1 / 8.9, 10 K 13.4 / 8.6,
    // 12 K 15.6 / 9.2, 16 K 19.2 / 14.4)
    p.wave_form = jwave < 0 ? p.nchunks > 1 : jwave > 0;
    if (p.wave_form) {
        p.bpc = std::max(1, std::min(B, jrows / p.rpb));
        p.nchunks = (B + p.bpc - 1) / p.bpc;
    }
    p.rch = (int)align_up((size_t)std::min<int64_t>(N, (int64_t)p.bpc * p.rpb), 8);
    return p;
}

RerankLayout make_layout(int64_t nq, int64_t ng, int d, int k1, int k2, int has_local) {
    RerankLayout L{};
    L.N = nq + ng;
    L.ld = (int64_t)align_up((size_t)L.N, 64);
    static_cast<RerankK &>(L) = clamp_k(L.N, k1, k2);
    WsCursor take;
    const size_t N = (size_t)L.N;
    L.feat = take(N * (size_t)d * 4);
    L.norms = take(N * 4);
    L.D = take(N * (size_t)L.ld * 4);
    L.MT = has_local ? take(N * (size_t)L.ld * 4) : L.D;
    L.rowmax = take(N * 4);
    L.rank = take(N * (size_t)L.KR * 4);
    L.rbits = take(N * (size_t)RB_WORDS * 4 * 2);  // two masks
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
    L.counters = take(64);
    L.total = take.off;
    return L;
}

// out[0] = sum of x[0..n) (one workgroup; statistics only)
__global__ __launch_bounds__(1024) void sum_i32_kernel(const int *__restrict__ x, int64_t n, unsigned long long *__restrict__ out) {
    __shared__ unsigned long long part[16];
    unsigned long long s = 0;
    for (int64_t i = threadIdx.x; i < n; i += 1024) s += (unsigned long long)(unsigned)x[i];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (int w = 0; w < 16; ++w) t += part[w];
        out[0] = t;
    }
}

void launch_sum_i32(const int *x, int64_t n, unsigned long long *out, hipStream_t stream) {
    hipLaunchKernelGGL(sum_i32_kernel, dim3(1), dim3(1024), 0, stream, x, n, out);
}

// ---------------------------------------------------------------------------------------------
// local query expansion (utils/reranking.py:73-78): V_qe[i] = fp16( sum_{m<k2} V[rank[i][m]] / k2 )
// fp32 sum in rank order, true divide by fp32(k2).  One wave per row.
// ---------------------------------------------------------------------------------------------
// V (vcnt/vidx/vval, row stride vcap) is global; ucnt / qcnt / qidx / qval are indexed by the local row
// Walk the sparse V rows of the first k2 neighbours of row i (one wave), f(c, hv) for every entry, neighbours in rank
// order.  The neighbour indices and their entry counts are fetched lane-parallel, and the first 64 entries of EIGHT
// neighbours are requested before the first is consumed (unconditional, clamped loads: counted waits) -- the plain loop
// paid three dependent memory round trips per neighbour, 45 per row and pass (4.0 ms at N = 100 000).
template <bool WITH_VAL, typename F>
__device__ __forceinline__ void qe_walk(const int *__restrict__ rank, int64_t i, int KR, int k2, const int *__restrict__ vcnt,
                                        const int *__restrict__ vidx, const uint16_t *__restrict__ vval, int vcap, int lane,
                                        F &&f) {
    for (int mb = 0; mb < k2; mb += 64) {
        const int mm = mb + lane;
        const int my_r = mm < k2 ? rank[i * KR + mm] : 0;
        const int my_cnt = mm < k2 ? vcnt[my_r] : 0;
        const int mtop = (k2 - mb < 64) ? k2 - mb : 64;
        for (int m0 = 0; m0 < mtop; m0 += 8) {
            int c[8], cn[8];
            uint16_t hv[8];
            int64_t rbase[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int sl = (m0 + u < mtop) ? m0 + u : m0;   // (wave-uniform) past the end: a copy of neighbour m0, count 0
                const int r = __builtin_amdgcn_readlane(my_r, sl);
                cn[u] = (m0 + u < mtop) ? __builtin_amdgcn_readlane(my_cnt, sl) : 0;
                rbase[u] = (int64_t)r * vcap;
                const int a = lane < cn[u] ? lane : 0;
                c[u] = vidx[rbase[u] + a];
                if (WITH_VAL) hv[u] = vval[rbase[u] + a];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if (lane < cn[u]) f(c[u], WITH_VAL ? hv[u] : (uint16_t)0);
                for (int a = lane + 64; a < cn[u]; a += 64)   // rows with more than 64 entries
                    f(vidx[rbase[u] + a], WITH_VAL ? vval[rbase[u] + a] : (uint16_t)0);
                if (WITH_VAL) __builtin_amdgcn_wave_barrier();
            }
        }
    }
}

__global__ __launch_bounds__(64) void qe_count_kernel(int64_t N, const int *__restrict__ rank, int KR, int k2,
                                                      const int *__restrict__ vcnt, const int *__restrict__ vidx,
                                                      int vcap, int *__restrict__ ucnt, int row0) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned *mask = (unsigned *)smem;
    const int nw = (int)((N + 31) >> 5);
    const int lane = threadIdx.x;
    const int li = blockIdx.x;
    const int i = row0 + li;
    for (int w = lane; w < nw; w += 64) mask[w] = 0u;
    __syncthreads();
    qe_walk<false>(rank, (int64_t)i, KR, k2, vcnt, vidx, nullptr, vcap, lane,
                   [&](int c, uint16_t) { atomicOr(&mask[c >> 5], 1u << (c & 31)); });
    __syncthreads();
    int tot = 0;
    for (int w = lane; w < nw; w += 64) tot += __popc(mask[w]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) tot += __shfl_xor(tot, off, 64);
    if (lane == 0) ucnt[li] = tot;
}

__global__ __launch_bounds__(64) void qe_fill_kernel(int64_t N, const int *__restrict__ rank, int KR, int k2,
                                                     const int *__restrict__ vcnt, const int *__restrict__ vidx,
                                                     const uint16_t *__restrict__ vval, int vcap, int qcap,
                                                     int *__restrict__ qcnt, int *__restrict__ qidx,
                                                     uint16_t *__restrict__ qval, int row0) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int nw = (int)((N + 31) >> 5);
    unsigned *mask = (unsigned *)smem;
    int *wpre = (int *)(mask + nw);
    float *acc = (float *)(wpre + nw);
    int *ulist = (int *)(acc + qcap);
    const int lane = threadIdx.x;
    const int li = blockIdx.x;
    const int i = row0 + li;
    for (int w = lane; w < nw; w += 64) mask[w] = 0u;
    for (int t = lane; t < qcap; t += 64) acc[t] = 0.0f;
    __syncthreads();
    qe_walk<false>(rank, (int64_t)i, KR, k2, vcnt, vidx, nullptr, vcap, lane,
                   [&](int c, uint16_t) { atomicOr(&mask[c >> 5], 1u << (c & 31)); });
    __syncthreads();
    // sorted union (np.unique) and, as a by-product of the same scan, the word prefix: slot(c) = wpre[c>>5] +
    // popc(mask[c>>5] & below(c))   (one pass over the N-bit mask instead of two)
    const int nU = extract_bits_sorted(mask, nw, ulist, lane, wpre);
    __syncthreads();
    // fp32 accumulation in rank order; one writer per slot and neighbour (a one-wave workgroup: its LDS operations
    // execute in program order)
    qe_walk<true>(rank, (int64_t)i, KR, k2, vcnt, vidx, vval, vcap, lane, [&](int c, uint16_t hv) {
        const int slot = wpre[c >> 5] + __popc(mask[c >> 5] & ((1u << (c & 31)) - 1u));
        acc[slot] = acc[slot] + h_to_f32(hv);
    });
    __syncthreads();
    const float k2f = (float)k2;
    int out = 0;
    for (int t0 = 0; t0 < nU; t0 += 64) {
        const int t = t0 + lane;
        uint16_t hv = 0;
        if (t < nU) hv = h_from_f32(__fdiv_rn(acc[t], k2f));
        const bool nz = (hv & 0x7fffu) != 0;
        const unsigned long long mm = __ballot(nz);
        if (nz) {
            const int p = out + __popcll(mm & ((1ull << lane) - 1ull));
            qidx[(int64_t)li * qcap + p] = ulist[t];
            qval[(int64_t)li * qcap + p] = hv;
        }
        out += __popcll(mm);
    }
    if (lane == 0) qcnt[li] = out;
}

// ---------------------------------------------------------------------------------------------
// inverted index (utils/reranking.py:80-82): CSC of V.  Order inside a column is irrelevant to
// the result (each row occurs once per column), so the fill uses atomic cursors.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void csc_count_kernel(int64_t N, const int *__restrict__ qcnt,
                                                        const int *__restrict__ qidx, int qcap,
                                                        unsigned *__restrict__ ccnt, int64_t row_lo) {
    const int lane = threadIdx.x & 63;
    const int64_t i = row_lo + (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= N) return;
    const int cnt = qcnt[i];
    for (int a = lane; a < cnt; a += 64) atomicAdd(&ccnt[qidx[i * qcap + a]], 1u);
}

// single-workgroup exclusive scan of ccnt[0..N) -> cptr[0..N]; also zeroes ccnt for reuse as cursor
__global__ __launch_bounds__(1024) void csc_scan_kernel(int64_t N, unsigned *__restrict__ ccnt,
                                                        long long *__restrict__ cptr) {
    __shared__ long long part[1024];
    const int tid = threadIdx.x;
    const int64_t per = (N + 1023) / 1024;
    const int64_t lo = (tid * per < N) ? tid * per : N, hi = (lo + per < N) ? lo + per : N;
    long long s = 0;
    for (int64_t c = lo; c < hi; ++c) s += ccnt[c];
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        long long run = 0;
        for (int t = 0; t < 1024; ++t) {
            const long long v = part[t];
            part[t] = run;
            run += v;
        }
        cptr[N] = run;
    }
    __syncthreads();
    long long run = part[tid];
    for (int64_t c = lo; c < hi; ++c) {
        cptr[c] = run;
        run += ccnt[c];
        ccnt[c] = 0u;
    }
}

__global__ __launch_bounds__(256) void csc_fill_kernel(int64_t N, const int *__restrict__ qcnt,
                                                       const int *__restrict__ qidx,
                                                       const uint16_t *__restrict__ qval, int qcap,
                                                       const long long *__restrict__ cptr,
                                                       unsigned *__restrict__ cursor, int *__restrict__ crow,
                                                       uint16_t *__restrict__ cval, int64_t row_lo) {
    const int lane = threadIdx.x & 63;
    const int64_t i = row_lo + (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= N) return;
    const int cnt = qcnt[i];
    for (int a = lane; a < cnt; a += 64) {
        const int c = qidx[i * qcap + a];
        const long long p = cptr[c] + (long long)atomicAdd(&cursor[c], 1u);
        crow[p] = (int)i;
        cval[p] = qval[i * qcap + a];
    }
}

// ---------------------------------------------------------------------------------------------
// Inverted index WITHOUT global atomics (the atomic-cursor build above ran at 1 % of HBM bandwidth: 25 M device-scope
// atomics for 12.5 M entries).  Counting sort with the rows cut into CSC_B blocks:
//   1. every block histograms the columns of its rows in LDS (LDS atomics) and writes its histogram row H[b][.]
//   2. per column: exclusive scan of H[.][c] over the blocks (in place) and the column total -> ccnt[c];
//      the existing single-workgroup scan turns ccnt into cptr
//   3. every block re-walks its rows with LDS cursors cptr[c] + H[b][c] and writes (row, value) to its slots
// Columns are processed in ranges of CSC_CR (LDS: 4 bytes per column) -- one range up to N = 36 864.
// The order of the rows inside a column depends on LDS-atomic arrival order within a block; the Jaccard sum does
// not (every row occurs once per column and owns its own accumulator).
// ---------------------------------------------------------------------------------------------
constexpr int CSC_B = 256, CSC_CR = 36864;
static_assert(CSC_B == 256, "the workspace layouts reserve 256 block histograms");
__global__ __launch_bounds__(1024) void csc2_hist_kernel(int64_t N, const int *__restrict__ qcnt, const int *__restrict__ qidx,
                                                         int qcap, int rows_per_block, unsigned *__restrict__ H,
                                                         int64_t row_lo, int64_t col_lo, int64_t col_hi) {
    // columns [col_lo, col_hi) only (the whole index: 0, N; a rank's column shard of the sharded build: its range)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned *hist = (unsigned *)smem;
    const int b = blockIdx.x;
    const int64_t c0 = col_lo + (int64_t)blockIdx.y * CSC_CR;
    const int cw = (int)((col_hi - c0 < CSC_CR) ? col_hi - c0 : CSC_CR);
    for (int c = threadIdx.x; c < cw; c += 1024) hist[c] = 0u;
    __syncthreads();
    const int64_t r_lo = row_lo + (int64_t)b * rows_per_block, r_hi = (r_lo + rows_per_block < N) ? r_lo + rows_per_block : N;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t i = r_lo + wave; i < r_hi; i += 16) {
        const int cnt = qcnt[i];
        for (int a = lane; a < cnt; a += 64) {
            const int64_t c = qidx[i * qcap + a] - c0;
            if (c >= 0 && c < cw) atomicAdd(&hist[c], 1u);
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < cw; c += 1024) H[(int64_t)b * N + c0 + c] = hist[c];
}
// per column: H[b][c] <- sum of H[b'][c] over b' < b; ccnt[c] = total
__global__ __launch_bounds__(256) void csc2_colscan_kernel(int64_t N, unsigned *__restrict__ H, unsigned *__restrict__ ccnt,
                                                           int64_t col_lo, int64_t col_hi) {
    const int64_t c = col_lo + (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= col_hi) return;
    unsigned run = 0u;
#pragma unroll 8
    for (int b = 0; b < CSC_B; ++b) {
        const unsigned v = H[(int64_t)b * N + c];
        H[(int64_t)b * N + c] = run;
        run += v;
    }
    ccnt[c] = run;
}
// cptr = exclusive scan of the column totals, in three fully parallel launches (the single-workgroup csc_scan_kernel
// above walks N / 1024 counts per thread at a stride and scans 1024 partial sums on one lane: 47 us at N = 20 000,
// 260 us at N = 100 000).  Tiles of 1024 columns.
__global__ __launch_bounds__(256) void scan_tile_sums_kernel(int64_t N, const unsigned *__restrict__ cnt,
                                                             unsigned long long *__restrict__ tile_sum) {
    __shared__ unsigned long long ws[4];
    const int64_t c0 = (int64_t)blockIdx.x * 1024 + threadIdx.x * 4;
    unsigned long long s = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) s += (c0 + u < N) ? cnt[c0 + u] : 0u;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
}
// tile_sum[0..nt) -> exclusive prefix in place; total -> cptr_end[0]
__global__ __launch_bounds__(1024) void scan_tile_bases_kernel(int nt, unsigned long long *__restrict__ tile_sum,
                                                               long long *__restrict__ cptr_end) {
    __shared__ unsigned long long ws[16];
    __shared__ unsigned long long carry;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (int t0 = 0; t0 < nt; t0 += 1024) {
        const int t = t0 + tid;
        const unsigned long long v = t < nt ? tile_sum[t] : 0ull;
        unsigned long long x = v;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned long long y = __shfl_up(x, off, 64);
            if (lane >= off) x += y;
        }
        if (lane == 63) ws[wave] = x;
        __syncthreads();
        unsigned long long wbase = 0;
        for (int w = 0; w < wave; ++w) wbase += ws[w];
        const unsigned long long base = carry;
        if (t < nt) tile_sum[t] = base + wbase + x - v;
        __syncthreads();
        if (tid == 1023) carry = base + wbase + x;
        __syncthreads();
    }
    if (tid == 0) cptr_end[0] = (long long)carry;
}
// cptr[c] = tile base + exclusive prefix inside the tile; cnt is zeroed for reuse as a cursor
__global__ __launch_bounds__(256) void scan_apply_kernel(int64_t N, unsigned *__restrict__ cnt,
                                                         const unsigned long long *__restrict__ tile_base,
                                                         long long *__restrict__ cptr) {
    __shared__ unsigned long long ws[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t c0 = (int64_t)blockIdx.x * 1024 + threadIdx.x * 4;
    unsigned v[4];
    unsigned long long s = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        v[u] = (c0 + u < N) ? cnt[c0 + u] : 0u;
        s += v[u];
    }
    unsigned long long x = s;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long y = __shfl_up(x, off, 64);
        if (lane >= off) x += y;
    }
    if (lane == 63) ws[wave] = x;
    __syncthreads();
    unsigned long long run = tile_base[blockIdx.x] + x - s;
    for (int w = 0; w < wave; ++w) run += ws[w];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        if (c0 + u < N) {
            cptr[c0 + u] = (long long)run;
            cnt[c0 + u] = 0u;
        }
        run += v[u];
    }
}

// chunk-boundary table of the Jaccard stage: HB[c][k] = absolute position (in crow / cval) of the first entry of column c
// that lies in row chunk k (= row block k * bpc), HB[c][nchunks] = end of the column.  One 8-byte read per (query,
// chunk, column) from a table of a few MB instead of four scattered reads of cptr and the [256][N] histograms.
__global__ __launch_bounds__(256) void csc2_bounds_kernel(int64_t N, int nchunks, int bpc, const unsigned *__restrict__ H,
                                                          const long long *__restrict__ cptr, unsigned *__restrict__ HB,
                                                          int64_t col_lo, int64_t col_hi) {
    const int64_t c = col_lo + (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= col_hi) return;
    const unsigned base = (unsigned)cptr[c];
    for (int k = 0; k < nchunks; ++k) HB[c * (nchunks + 1) + k] = base + H[(int64_t)k * bpc * N + c];
    HB[c * (nchunks + 1) + nchunks] = (unsigned)cptr[c + 1];
}
__global__ __launch_bounds__(1024) void csc2_fill_kernel(int64_t N, const int *__restrict__ qcnt, const int *__restrict__ qidx,
                                                         const uint16_t *__restrict__ qval, int qcap, int rows_per_block,
                                                         const unsigned *__restrict__ H, const long long *__restrict__ cptr,
                                                         unsigned *__restrict__ cpk, int64_t row_lo, int blocks_per_chunk,
                                                         int64_t col_lo, int64_t col_hi) {
    // entries are PACKED: (row - first row of the Jaccard chunk the row block belongs to) << 16 | fp16 bits of V_qe
    // (a chunk has at most 24 K rows): 4 bytes per entry in ONE array instead of 4 + 2 in two -- a third fewer bytes
    // and, at large N, ~40 % fewer 128-byte lines per gathered sub-range
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned *cur = (unsigned *)smem;
    const int b = blockIdx.x;
    const int64_t c0 = col_lo + (int64_t)blockIdx.y * CSC_CR;
    const int cw = (int)((col_hi - c0 < CSC_CR) ? col_hi - c0 : CSC_CR);
    for (int c = threadIdx.x; c < cw; c += 1024) cur[c] = (unsigned)cptr[c0 + c] + H[(int64_t)b * N + c0 + c];
    __syncthreads();
    const int64_t r_lo = row_lo + (int64_t)b * rows_per_block, r_hi = (r_lo + rows_per_block < N) ? r_lo + rows_per_block : N;
    const int64_t chunk_row0 = row_lo + (int64_t)(b / blocks_per_chunk) * blocks_per_chunk * rows_per_block;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t i = r_lo + wave; i < r_hi; i += 16) {
        const int cnt = qcnt[i];
        for (int a = lane; a < cnt; a += 64) {
            const int64_t c = qidx[i * qcap + a] - c0;
            if (c >= 0 && c < cw) {
                const unsigned p = atomicAdd(&cur[c], 1u);
                cpk[p] = ((unsigned)(i - chunk_row0) << 16) | (unsigned)qval[i * qcap + a];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Jaccard min-sum with fp16 accumulation in ascending column order + final blend
// (utils/reranking.py:84-100).  One 256-thread workgroup per query; t[] lives in LDS as fp16 bits,
// r-space processed in chunks of rch entries so that any N fits.
// ---------------------------------------------------------------------------------------------
// Two forms (jaccard_plan): 256 threads per (query, chunk of <= 24 K rows) with one barrier per column -- whole columns
// when N - nq <= 24 576 -- and ONE wave per (query, chunk of ~8 K rows) without barriers when the 256-thread form would need
// several chunks (N = 100 000: 45.5 -> 33.8 ms, MSMT17 shape 21.8 -> 18.6 ms, with the counted waits, the register-held
// column table and the branch-free accumulation below; the same one-wave split measured 41 / 25 ms before those).
constexpr int JT = 256; // threads per query workgroup (multi-wave form)
// NPF entries per thread and column are held in registers (columns up to NPF * JT entries; longer ones take the direct
// path below), the gathers of PD columns are in flight.  <2, 4> suits whole columns (~600 entries: 43 KB in flight per CU
// at three workgroups); at large N a workgroup sees ~130-entry sub-ranges and <1, 12> keeps as many bytes in flight.
template <int JT_, int NPF, int PD, bool PACKED>
__global__ __launch_bounds__(JT_) void jaccard_kernel(int64_t N, int64_t nq, const float *__restrict__ MT, int64_t ld,
                                                      const float *__restrict__ rowmax,
                                                      const int *__restrict__ qcnt, const int *__restrict__ qidx,
                                                      const uint16_t *__restrict__ qval, int qcap,
                                                      const long long *__restrict__ cptr,
                                                      const int *__restrict__ crow, const uint16_t *__restrict__ cval,
                                                      int rch, uint16_t one_minus_lam_h, float lam32,
                                                      float *__restrict__ out, int64_t ldo,
                                                      unsigned long long *__restrict__ pair_counter, int q0,
                                                      const unsigned *__restrict__ H, int rows_per_block,
                                                      int blocks_per_chunk, int dbg) {
    // H != NULL (inverted index built by csc2_*: the entries of a column are grouped by row block; H = the chunk
    // boundaries of every column): blockIdx.y selects a chunk of blocks_per_chunk row blocks = rch rows, and the
    // workgroup gathers exactly the sub-range of every column that lies in it.  (Round 1 walked the r-space chunk by chunk inside one workgroup and re-read every column in
    // full for every chunk: 3x the gather traffic at N = 100 000, at one workgroup per CU.)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint16_t *t = (uint16_t *)smem;                                   // [rch]
    long long *cp0 = (long long *)(smem + align_up((size_t)rch * 2 + 16, 16)); // [cnt]  (t[rch] = dummy slot)
    int *clen = (int *)(cp0 + qcap);                                  // [cnt]
    uint16_t *vi = (uint16_t *)(clen + qcap);                         // [cnt]
    const int tid = threadIdx.x;
    const int64_t i = blockIdx.x;              // local query row: MT / rowmax / out are indexed by it
    const int64_t ig = (int64_t)q0 + i;        // global row: the sparse V rows are indexed by it
    const int cnt = qcnt[ig];
    unsigned long long pairs = 0;
    const int b_lo = H ? (int)blockIdx.y * blocks_per_chunk : 0;
    const int b_hi = b_lo + blocks_per_chunk;   // >= CSC_B for the last chunk
    const int nb1 = (int)gridDim.y + 1;
    for (int a = tid; a < cnt; a += JT_) {
        const int c = qidx[ig * qcap + a];
        long long p0, p1;
        if (H) {   // H = chunk-boundary table [N][nchunks + 1] (csc2_bounds_kernel)
            p0 = H[(int64_t)c * nb1 + blockIdx.y];
            p1 = H[(int64_t)c * nb1 + blockIdx.y + 1];
        } else {
            p0 = cptr[c];
            p1 = cptr[c + 1];
        }
        cp0[a] = p0;
        clen[a] = (int)(p1 - p0);
        vi[a] = qval[ig * qcap + a];
        pairs += (unsigned long long)(p1 - p0);
    }
    if (pair_counter) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) pairs += __shfl_xor(pairs, off, 64);
        if ((tid & 63) == 0 && pairs) atomicAdd(pair_counter, pairs);
    }
    const float mx = rowmax[i];
    const float *row = MT + i * ld;
    const uint16_t H1 = 0x3c00u, H2 = 0x4000u;
    const unsigned long long last = cnt > 0 ? (unsigned long long)(cptr[N] - 1) : 0ull;   // cnt > 0: the index is not empty
    // the inverted index holds the rows [nq, N) only (launch_csc): the accumulators start at row nq
    const int64_t r_first = nq + (H ? (int64_t)b_lo * rows_per_block : 0);
    const int64_t r_end = nq + (int64_t)b_hi * rows_per_block;
    const int64_t r_last = H ? (r_end < N ? r_end : N) : N;   // (rch, the LDS size, may be rounded up past it)
    for (int64_t r0 = r_first; r0 < r_last; r0 += rch) {
        const int64_t r1 = (r0 + rch < r_last) ? r0 + rch : r_last;
        for (int r = tid; r < rch; r += JT_) t[r] = 0;
        __syncthreads();
        const int r0i = (int)r0;
        const unsigned span = (unsigned)(r1 - r0);
        // ascending column; rows of one column are distinct, so the threads of a column never collide and
        // one barrier per column keeps the fp16 accumulation order of the reference.  The (row, value)
        // pairs of column a+1 are requested into registers before column a is applied, so the L2/HBM
        // latency of the gathers is paid once per pipeline fill instead of once per column.
        // the (row, value) pairs of columns a+1 .. a+PD are requested before column a is applied (one column ahead
        // left ~1.6 us per column exposed: a barrier plus most of an L2 / HBM round trip)
        // Every gather is UNCONDITIONAL (clamped column index, entry 0 for the lanes past the column's end) and a
        // column's registers are refilled only after it has been applied: hipcc then counts the loads in flight exactly
        // and waits with vmcnt((PD - 1) * 2 * NPF).  (With the loads under `if (e < len)` / `if (a + PD < cnt)` it could
        // not know how many younger loads exist, and with the refill issued before the apply it rotated the registers
        // by moves at the loop end: both forms drained to vmcnt(0) once per PD columns -- a full HBM round trip per
        // group, ~0.8 us per column.)
        // The column table (start, length, V[i][c]) is NOT read from LDS per column -- four dependent LDS round trips per
        // step were most of a step's time at one or two waves per SIMD -- but once per 64 columns: lane l keeps the
        // entries of column 64 b + l in registers (one set for the column being applied, one for the column being
        // prefetched, PD columns ahead) and a step picks its column with v_readlane.
        static_assert(64 % PD == 0, "batch boundaries must fall on group boundaries");
        int pr[PD][NPF];
        uint16_t pv[PD][NPF];
        const int lane = tid & 63;
        unsigned f_lo = 0, f_hi = 0;
        int f_len = 0, a_len = 0, a_vi = 0;
        auto load_fetch_batch = [&](int base) {
            int idx = base + lane;
            idx = idx < cnt ? idx : cnt - 1;
            const unsigned long long p0 = (unsigned long long)cp0[idx];
            f_lo = (unsigned)p0;
            f_hi = (unsigned)(p0 >> 32);
            f_len = clen[idx];
        };
        auto load_apply_batch = [&](int base) {
            int idx = base + lane;
            idx = idx < cnt ? idx : cnt - 1;
            a_len = clen[idx];
            a_vi = vi[idx];
        };
        // (the loads use a wave-uniform base + a 32-bit lane offset; lanes past the column's end read its first entry
        // -- `last` keeps that in bounds for an empty column at the very end of the index -- and are masked when applied)
        auto fetch = [&](int a, int (&er)[NPF], uint16_t (&ev)[NPF]) {   // a >= cnt: the batch entry is a clamped copy
            const int sl = a & 63;
            unsigned long long p0 = (unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)f_lo, sl) |
                                    ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)f_hi, sl) << 32);
            p0 = p0 < last ? p0 : last;
            const int len = __builtin_amdgcn_readlane(f_len, sl);
            const int *cb = crow + p0;
            const uint16_t *vb = cval + p0;
#pragma unroll
            for (int k = 0; k < NPF; ++k) {
                const unsigned e = (unsigned)(tid + k * JT_);
                const unsigned off = e < (unsigned)len ? e : 0u;
                er[k] = cb[off];
                if (!PACKED) ev[k] = vb[off];
            }
        };
        if (cnt > 0) {
            load_fetch_batch(0);
#pragma unroll
            for (int d = 0; d < PD; ++d) fetch(d, pr[d], pv[d]);
        }
        for (int a0 = 0; a0 < cnt; a0 += PD) {
            if ((a0 & 63) == 0) load_apply_batch(a0);
            if (((a0 + PD) & 63) == 0) load_fetch_batch(a0 + PD);
#pragma unroll
            for (int d = 0; d < PD; ++d) {
                const int a = a0 + d;
                if (a < cnt) {
                    const uint16_t vic = (uint16_t)__builtin_amdgcn_readlane(a_vi, a & 63);
                    const int len = __builtin_amdgcn_readlane(a_len, a & 63);
                    // branch free: lanes without an entry in this chunk add into a dummy slot behind the accumulators
                    // (the NPF entries of a lane belong to one column, i.e. to different rows: read all accumulators,
                    // then add, then write -- one LDS round trip per column instead of NPF)
                    unsigned idx[NPF];
                    uint16_t tv[NPF];
#pragma unroll
                    for (int k = 0; k < NPF; ++k) {
                        // PACKED: chunk-relative row in the high half (every entry of the sub-range lies in the chunk)
                        const unsigned rl = PACKED ? ((unsigned)pr[d][k] >> 16) : (unsigned)(pr[d][k] - r0i);
                        const bool ok = (tid + k * JT_ < len) && (PACKED || rl < span) && !(dbg & 1);
                        idx[k] = ok ? rl : (unsigned)(rch + k);   // NPF dummy slots
                        tv[k] = t[idx[k]];
                    }
#pragma unroll
                    for (int k = 0; k < NPF; ++k) {
                        const uint16_t vv = PACKED ? (uint16_t)((unsigned)pr[d][k] & 0xffffu) : pv[d][k];
                        t[idx[k]] = h_add_native(tv[k], mpreid_h_min_nonneg(vic, vv));
                    }
                    if (len > NPF * JT_ && !(dbg & 8)) { // rare long column: the tail is gathered directly
                        const long long p0 = cp0[a];
                        for (int e = tid + NPF * JT_; e < len; e += JT_) {
                            if (PACKED) {
                                const unsigned pe = (unsigned)crow[p0 + e];
                                const uint16_t m = mpreid_h_min_nonneg(vic, (uint16_t)(pe & 0xffffu));
                                t[pe >> 16] = h_add_native(t[pe >> 16], m);
                            } else {
                                const int r = crow[p0 + e];
                                if (r >= r0 && r < r1) {
                                    const uint16_t m = mpreid_h_min_nonneg(vic, cval[p0 + e]);
                                    t[r - r0] = h_add_native(t[r - r0], m);
                                }
                            }
                        }
                    }
                }
                fetch(a + PD, pr[d], pv[d]);
                __syncthreads();
            }
        }
        const int64_t jlo = (r0 > nq) ? r0 : nq;
        // eight independent loads per thread and trip (a one-wave workgroup would otherwise pay a memory round trip per
        // 64 elements)
        for (int64_t jb = jlo; jb < ((dbg & 4) ? jlo : r1); jb += 8 * JT_) {
            float dv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int64_t j = jb + u * JT_ + tid;
                dv[u] = row[j < r1 ? j : r1 - 1];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int64_t j = jb + u * JT_ + tid;
                if (j < r1) {
                    const uint16_t tv = t[j - r0];
                    const uint16_t den = h_sub_native(H2, tv);
                    const uint16_t qt = h_div_native(tv, den);
                    const uint16_t jac = h_sub_native(H1, qt);
                    const uint16_t jl = h_mul_native(jac, one_minus_lam_h);
                    const float o = __fdiv_rn(dv[u], mx);
                    out[i * ldo + (j - nq)] = h_to_f32(jl) + o * lam32;
                }
            }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------
// One-wave form of the Jaccard stage WITHOUT a column table in LDS (blocked + packed index only): the workgroup's LDS is
// the fp16 accumulators of its row chunk and nothing else (16 KB at 8 K rows: nine workgroups per CU instead of six), and
// the per-column data (start of the sub-range, its length, V[i][c]) live in lane registers, 64 columns at a time:
//   cur  = the batch the column being applied is in, nxt = the following batch (the prefetch stream, PD columns ahead,
//   may already be there), both fully resolved (position / length from the chunk-boundary table HB);
//   c2 / v2 = column indices and values of the batch after that, loaded one batch early so that resolving them at the
//   next rotation is one round trip that nothing waits for.
// In-kernel stamps of the table form at N = 100 000 (per (query, chunk) workgroup, cycles): table set-up 29 k, zeroing
// 9 k, column loop 325 k (489 per column at 1.5 waves per SIMD), output pass 69 k.
// ---------------------------------------------------------------------------------------------
template <int JT_, int NPF, int PD>
__global__ __launch_bounds__(JT_) void jaccard_wave_kernel(int64_t N, int64_t nq, const float *__restrict__ MT, int64_t ld,
                                                          const float *__restrict__ rowmax, const int *__restrict__ qcnt,
                                                          const int *__restrict__ qidx, const uint16_t *__restrict__ qval,
                                                          int qcap, const long long *__restrict__ cptr,
                                                          const unsigned *__restrict__ cpk, int rch,
                                                          uint16_t one_minus_lam_h, float lam32, float *__restrict__ out,
                                                          int64_t ldo, unsigned long long *__restrict__ pair_counter, int q0,
                                                          const unsigned *__restrict__ HB, int rows_per_block,
                                                          int blocks_per_chunk) {
    static_assert(64 % PD == 0, "batch boundaries must fall on group boundaries");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint16_t *t = (uint16_t *)smem;            // [rch] + NPF dummy slots
    const int tid = threadIdx.x, lane = tid & 63;
    constexpr bool MULTI = JT_ > 64;   // several waves: one barrier per column keeps the accumulation order
    const int64_t i = blockIdx.x;              // local query row: MT / rowmax / out are indexed by it
    const int64_t ig = (int64_t)q0 + i;        // global row: the sparse V rows are indexed by it
    const int y = (int)blockIdx.y, nb1 = (int)gridDim.y + 1;
    const int cnt = qcnt[ig];
    const int64_t r0 = nq + (int64_t)y * blocks_per_chunk * rows_per_block;
    const int64_t r_end = r0 + (int64_t)blocks_per_chunk * rows_per_block;
    const int64_t r1 = r_end < N ? r_end : N;
    for (int r = tid; r < rch + 8; r += JT_) t[r] = 0;
    if (MULTI) __syncthreads();
    const unsigned last = cnt > 0 ? (unsigned)(cptr[N] - 1) : 0u;   // cnt > 0: the index is not empty
    unsigned pairs = 0;
    // column indices / values of a batch (lanes past the end: a copy of the last column, marked by v >> 31)
    auto load_cols = [&](int base, int &c, unsigned &v) {
        const int idx = base + lane;
        const int ic = idx < cnt ? idx : cnt - 1;
        c = qidx[ig * qcap + ic];
        v = (unsigned)qval[ig * qcap + ic] | (idx < cnt ? 0u : 0x80000000u);
    };
    // start (clamped into the index) and (length << 16 | V[i][c]) of the chunk's sub-range of every column of a batch
    auto resolve = [&](int c, unsigned v, unsigned &p0, unsigned &lenvi) {
        const unsigned a = HB[(int64_t)c * nb1 + y], b = HB[(int64_t)c * nb1 + y + 1];
        const unsigned len = (v >> 31) ? 0u : b - a;
        p0 = a < last ? a : last;
        lenvi = (len << 16) | (v & 0xffffu);
        pairs += len;
    };
    if (cnt > 0) {
        unsigned cur_p0, cur_lv, nxt_p0, nxt_lv, v2;
        int c2;
        {
            int c0, c1;
            unsigned v0, v1;
            load_cols(0, c0, v0);
            load_cols(64, c1, v1);
            load_cols(128, c2, v2);
            resolve(c0, v0, cur_p0, cur_lv);
            resolve(c1, v1, nxt_p0, nxt_lv);
        }
        unsigned pr[PD][NPF];
        // (wave-uniform base + 32-bit lane offset; lanes past the column's end read its first entry and are masked when
        // applied; every gather is unconditional so that hipcc counts the loads in flight exactly)
        auto fetch = [&](unsigned p0v, unsigned lvv, int a, unsigned (&er)[NPF]) {
            const int sl = a & 63;
            const unsigned p0 = (unsigned)__builtin_amdgcn_readlane((int)p0v, sl);
            const unsigned len = (unsigned)__builtin_amdgcn_readlane((int)lvv, sl) >> 16;
            const unsigned *cb = cpk + p0;
#pragma unroll
            for (int k = 0; k < NPF; ++k) {
                const unsigned e = (unsigned)(tid + k * JT_);
                er[k] = cb[e < len ? e : 0u];
            }
        };
#pragma unroll
        for (int d = 0; d < PD; ++d) fetch(cur_p0, cur_lv, d, pr[d]);
        for (int a0 = 0; a0 < cnt; a0 += PD) {
            if ((a0 & 63) == 0 && a0 > 0) {   // the apply stream enters the next batch
                cur_p0 = nxt_p0;
                cur_lv = nxt_lv;
                resolve(c2, v2, nxt_p0, nxt_lv);
                load_cols(a0 + 128, c2, v2);
            }
            // the prefetch stream (columns a0 + PD ...) is in the next batch during the last group of a batch
            const bool f_nxt = ((a0 + PD) >> 6) != (a0 >> 6);
            const unsigned f_p0 = f_nxt ? nxt_p0 : cur_p0, f_lv = f_nxt ? nxt_lv : cur_lv;
#pragma unroll
            for (int d = 0; d < PD; ++d) {
                const int a = a0 + d;
                if (a < cnt) {
                    const unsigned lv = (unsigned)__builtin_amdgcn_readlane((int)cur_lv, a & 63);
                    const uint16_t vic = (uint16_t)(lv & 0xffffu);
                    const unsigned len = lv >> 16;
                    // branch free: lanes without an entry add into a dummy slot behind the accumulators; the NPF entries of
                    // a lane belong to one column, i.e. to different rows: read all accumulators, add, write
                    unsigned idx[NPF];
                    uint16_t tv[NPF];
#pragma unroll
                    for (int k = 0; k < NPF; ++k) {
                        idx[k] = ((unsigned)(tid + k * JT_) < len) ? (pr[d][k] >> 16) : (unsigned)(rch + k);
                        tv[k] = t[idx[k]];
                    }
#pragma unroll
                    for (int k = 0; k < NPF; ++k)
                        t[idx[k]] = h_add_native(tv[k], mpreid_h_min_nonneg(vic, (uint16_t)(pr[d][k] & 0xffffu)));
                    if (len > (unsigned)(NPF * JT_)) {   // long sub-range: the tail is gathered directly
                        const unsigned p0 = (unsigned)__builtin_amdgcn_readlane((int)cur_p0, a & 63);
                        for (unsigned e = (unsigned)(tid + NPF * JT_); e < len; e += JT_) {
                            const unsigned pe = cpk[p0 + e];
                            t[pe >> 16] = h_add_native(t[pe >> 16], mpreid_h_min_nonneg(vic, (uint16_t)(pe & 0xffffu)));
                        }
                    }
                }
                fetch(f_p0, f_lv, a + PD, pr[d]);
                if (MULTI) __syncthreads();
            }
        }
    }
    if (MULTI) __syncthreads();
    if (pair_counter && tid < 64) {   // (every wave resolves the same columns: wave 0 reports)
        unsigned long long ps = pairs;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) ps += __shfl_xor(ps, off, 64);
        if (lane == 0 && ps) atomicAdd(pair_counter, ps);
    }
    // blend: final = fp32(fp16(J * fp16(1 - lambda))) + O[i][j] * lambda for the chunk's gallery columns
    const float mx = rowmax[i];
    const float *row = MT + i * ld;
    const uint16_t H1 = 0x3c00u, H2 = 0x4000u;
    constexpr int OU = 16;   // independent loads per thread and trip
    for (int64_t jb = r0; jb < r1; jb += OU * JT_) {
        float dv[OU];
#pragma unroll
        for (int u = 0; u < OU; ++u) {
            const int64_t j = jb + u * JT_ + tid;
            dv[u] = row[j < r1 ? j : r1 - 1];
        }
#pragma unroll
        for (int u = 0; u < OU; ++u) {
            const int64_t j = jb + u * JT_ + tid;
            if (j < r1) {
                const uint16_t tv = t[j - r0];
                const uint16_t den = h_sub_native(H2, tv);
                const uint16_t qt = h_div_native(tv, den);
                const uint16_t jac = h_sub_native(H1, qt);
                const uint16_t jl = h_mul_native(jac, one_minus_lam_h);
                const float o = __fdiv_rn(dv[u], mx);
                out[i * ldo + (j - nq)] = h_to_f32(jl) + o * lam32;
            }
        }
    }
}

uint16_t f64_to_f16_host(double d) {
    // single rounding double -> half (numpy casts the Python float 1 - lambda straight to float16)
    if (d != d) return 0x7e00u;
    uint16_t sign = 0;
    if (d < 0 || (d == 0 && 1.0 / d < 0)) {
        sign = 0x8000u;
        d = -d;
    }
    if (d >= 65520.0) return (uint16_t)(sign | 0x7c00u);
    if (d == 0.0) return sign;
    int e;
    (void)frexp(d, &e);
    const int ue = e - 1;
    const double q = (ue < -14) ? ldexp(1.0, -24) : ldexp(1.0, ue - 10);
    const double r = nearbyint(d / q) * q;
    return (uint16_t)(sign | mpreid_f32_to_f16((float)r));
}

// The two documented limits of DENSE (include/mpreid.h "Limits"), in one place: the launchers refuse by them and
// mpreid_rerank_fits answers by them.
static bool dense_kr_ok(const RerankLayout &L) { return L.KR <= RB_WORDS * 32; }   // 256: sel[] / the reciprocity masks
static bool dense_lds_ok(const RerankLayout &L) {
    return krecip_lds_bytes(false, (int)((L.N + 31) >> 5), L.K, L.vcap, 0) <= LDS_WG_MAX;
}

// (7) query expansion of the rows [row0, row0 + rows) from the V rows of all N: union sizes, then the fill with row
// stride qcap >= the largest union
static int launch_qe_count(int64_t N, const int *rank, int KR, int k2, int64_t row0, int64_t rows, const int *vcnt,
                    const int *vidx, int vcap, int *ucnt, hipStream_t stream) {
    const size_t lds = (size_t)((N + 31) >> 5) * 4;
    int rc = mpreid_dyn_lds(qe_count_kernel, lds);
    if (rc) return rc;
    hipLaunchKernelGGL(qe_count_kernel, dim3((unsigned)rows), dim3(64), lds, stream, N, rank, KR, k2, vcnt, vidx, vcap, ucnt,
                       (int)row0);
    LAUNCH_CHECK();
    return MPREID_OK;
}

static int launch_qe_fill(int64_t N, const int *rank, int KR, int k2, int64_t row0, int64_t rows, const int *vcnt,
                   const int *vidx, const uint16_t *vval, int vcap, int qcap, int *qcnt, int *qidx, uint16_t *qval,
                   hipStream_t stream) {
    const size_t lds = (size_t)((N + 31) >> 5) * 8 + (size_t)qcap * 8;
    int rc = mpreid_dyn_lds(qe_fill_kernel, lds);
    if (rc) return rc;
    hipLaunchKernelGGL(qe_fill_kernel, dim3((unsigned)rows), dim3(64), lds, stream, N, rank, KR, k2, vcnt, vidx, vval, vcap, qcap,
                       qcnt, qidx, qval, (int)row0);
    LAUNCH_CHECK();
    return MPREID_OK;
}

// max of x[0..n) -> out[0] (one workgroup)
__global__ __launch_bounds__(1024) void max_i32_kernel(const int *__restrict__ x, int64_t n, int *__restrict__ out) {
    __shared__ int part[16];
    int m = 0;
    for (int64_t i = threadIdx.x; i < n; i += 1024) m = max(m, x[i]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = max(m, __shfl_xor(m, off, 64));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 16; ++w) m = max(m, part[w]);
        out[0] = m;
    }
}

void launch_max_i32(const int *x, int64_t n, int *out, hipStream_t stream) {
    hipLaunchKernelGGL(max_i32_kernel, dim3(1), dim3(1024), 0, stream, x, n, out);
}

// the blocked inverted index addresses its packed entries with 32 bits
static bool csc_packed_ok(int64_t n, int qstride) { return (uint64_t)n * (uint64_t)qstride < (1ull << 32); }

// The blocked (atomics-free) build of the columns [c_lo, c_hi), first half: ccnt[c] = number of indexed entries (rows
// [nq, n)) of every column of the window; chist keeps the per-block offsets of those columns for the second half.
static int csc_blocked_count(int64_t n, int64_t nq, const int *qcnt, const int *qidx, int qstride, int64_t c_lo, int64_t c_hi,
                      unsigned *chist, unsigned *ccnt, hipStream_t stream) {
    const JaccardPlan jp = jaccard_plan(n - nq);
    const int64_t cols = c_hi - c_lo;
    const int nranges = (int)((cols + CSC_CR - 1) / CSC_CR);
    const size_t lds = (size_t)std::min<int64_t>(cols, CSC_CR) * 4;
    int rc = mpreid_dyn_lds(csc2_hist_kernel, lds);
    if (rc) return rc;
    hipLaunchKernelGGL(csc2_hist_kernel, dim3(CSC_B, nranges), dim3(1024), lds, stream, n, qcnt, qidx, qstride, jp.rpb, chist, nq,
                       c_lo, c_hi);
    hipLaunchKernelGGL(csc2_colscan_kernel, dim3((unsigned)((cols + 255) / 256)), dim3(256), 0, stream, n, chist, ccnt, c_lo, c_hi);
    return MPREID_OK;
}

// Second half: cptr[0 .. n] = exclusive scan of the counts of ALL columns (ccnt_all is zeroed: scratch), then the packed
// entries of the columns [c_lo, c_hi) at their global positions cpk[cptr[c_lo] .. cptr[c_hi]) and the rows [c_lo, c_hi) of
// the chunk-boundary table hb.  chist: as the first half left it; the tile sums of the scan sit behind its bounds table.
static int csc_blocked_fill(int64_t n, int64_t nq, const int *qcnt, const int *qidx, const uint16_t *qval, int qstride, int64_t c_lo,
                     int64_t c_hi, unsigned *ccnt_all, unsigned *chist, long long *cptr, unsigned *cpk, unsigned *hb,
                     hipStream_t stream) {
    const JaccardPlan jp = jaccard_plan(n - nq);
    const int nt = (int)((n + 1023) / 1024);
    unsigned long long *tsum = (unsigned long long *)((char *)chist + align_up((size_t)n * (CSC_B + 257) * 4, 8));
    hipLaunchKernelGGL(scan_tile_sums_kernel, dim3((unsigned)nt), dim3(256), 0, stream, n, ccnt_all, tsum);
    hipLaunchKernelGGL(scan_tile_bases_kernel, dim3(1), dim3(1024), 0, stream, nt, tsum, cptr + n);
    hipLaunchKernelGGL(scan_apply_kernel, dim3((unsigned)nt), dim3(256), 0, stream, n, ccnt_all, tsum, cptr);
    if (c_hi > c_lo) {
        const int64_t cols = c_hi - c_lo;
        const int nranges = (int)((cols + CSC_CR - 1) / CSC_CR);
        const size_t lds = (size_t)std::min<int64_t>(cols, CSC_CR) * 4;
        int rc = mpreid_dyn_lds(csc2_fill_kernel, lds);
        if (rc) return rc;
        hipLaunchKernelGGL(csc2_fill_kernel, dim3(CSC_B, nranges), dim3(1024), lds, stream, n, qcnt, qidx, qval, qstride, jp.rpb,
                           chist, cptr, cpk, nq, jp.bpc, c_lo, c_hi);
        hipLaunchKernelGGL(csc2_bounds_kernel, dim3((unsigned)((cols + 255) / 256)), dim3(256), 0, stream, n, jp.nchunks, jp.bpc,
                           chist, cptr, hb, c_lo, c_hi);
    }
    return MPREID_OK;
}

// The round-1 build with global atomic cursors, over the rows [nq, N) of the ELL matrix with row stride fcap.
int launch_csc_atomic(int64_t N, int64_t nq, const int *fcnt, const int *fidx, const uint16_t *fval, int fcap, unsigned *ccnt,
                      long long *cptr, int *crow, uint16_t *cval, hipStream_t stream) {
    const int64_t M = N - nq;   // indexed rows
    HIP_TRY(hipMemsetAsync(ccnt, 0, (size_t)(N + 1) * 4, stream));
    hipLaunchKernelGGL(csc_count_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, stream, N, fcnt, fidx, fcap, ccnt, nq);
    hipLaunchKernelGGL(csc_scan_kernel, dim3(1), dim3(1024), 0, stream, N, ccnt, cptr);
    hipLaunchKernelGGL(csc_fill_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, stream, N, fcnt, fidx, fval, fcap, cptr,
                       ccnt, crow, cval, nq);
    return MPREID_OK;
}

// inverted index of the ELL rows (fcnt, fidx, fval; row stride qcap) -> cptr / crow / cval, over the rows [nq, N) ONLY:
// the Jaccard stage produces final_dist[:nq, nq:], i.e. the accumulators of the first nq rows are never read (the
// reference computes and discards them, utils/reranking.py:84-100) -- a fifth of the entries, gathers and accumulator
// rows at nq = N / 5.  With a block-histogram buffer (chist: [CSC_B][N] u32 + the chunk-boundary table) the atomics-free
// counting sort over CSC_B blocks of the indexed rows is used (and *blocked = true: the Jaccard stage then gathers
// exact sub-ranges per row chunk); otherwise the round-1 atomic build.
static int launch_csc(int64_t N, int64_t nq, const int *fcnt, const int *fidx, const uint16_t *fval, int qcap, unsigned *ccnt,
               unsigned *chist, long long *cptr, int *crow, uint16_t *cval, hipStream_t stream, bool *blocked) {
    static const bool csc_atomic = mpreid_tune("csc_atomic", 0) != 0;   // A/B switch: the round-1 atomic build
    const bool blocked_csc = chist && !csc_atomic && csc_packed_ok(N, qcap);
    *blocked = blocked_csc;
    int rc;
    if (blocked_csc) {   // all columns; the packed entries live in the crow buffer, the bounds table behind the histograms
        rc = csc_blocked_count(N, nq, fcnt, fidx, qcap, 0, N, chist, ccnt, stream);
        if (rc) return rc;
        rc = csc_blocked_fill(N, nq, fcnt, fidx, fval, qcap, 0, N, ccnt, chist, cptr, (unsigned *)crow, chist + (size_t)N * CSC_B,
                              stream);
    } else {
        rc = launch_csc_atomic(N, nq, fcnt, fidx, fval, qcap, ccnt, cptr, crow, cval, stream);
    }
    if (rc) return rc;
    LAUNCH_CHECK();
    return MPREID_OK;
}

// Jaccard + blend for the query rows [q0, q0 + qrows): MT / rowmax / out indexed by the local row
static int launch_jaccard(int64_t N, int64_t nq, int q0, int64_t qrows, const float *MT, int64_t ld, const float *rowmax,
                          const int *fcnt, const int *fidx, const uint16_t *fval, int qcap, const long long *cptr,
                          const int *crow, const uint16_t *cval, const unsigned *chist, bool blocked, double lambda_value,
                          float *out, int64_t ldo, unsigned long long *pair_counter, hipStream_t stream,
                          const unsigned *bounds = nullptr) {   // bounds: the chunk-boundary table when it does not sit behind chist
    const uint16_t oml = f64_to_f16_host(1.0 - lambda_value);
    const float lam32 = (float)lambda_value;
    int rch = (int)std::min<int64_t>(N - nq, 49152);
    rch = (int)align_up((size_t)rch, 8);
    const unsigned *Hp = nullptr;
    int rpb = 0, bpc = 0, nchunks = 1, threads = JT;
    if (blocked) {
        const JaccardPlan jp = jaccard_plan(N - nq);
        rpb = jp.rpb; bpc = jp.bpc; nchunks = jp.nchunks; rch = jp.rch;
        threads = jp.wave_form ? 64 : JT;
        Hp = bounds ? bounds : chist + (size_t)N * CSC_B;   // the chunk-boundary table
    }
    // timing ablations (wrong results): 1 nothing is accumulated, 4 no output pass, 8 no direct path for long columns.
    // (An ablation that points every gather at ONE address measures an L2 hot spot, not the loop: removed.)
    // Compiled in only with -DMPREID_ABLATION (never in the shipped library: a stray environment variable must not be
    // able to change results).
    static const int jdbg = mpreid_ablation_env("MPREID_JACCARD_DBG");
    const size_t lds = align_up((size_t)rch * 2 + 16, 16) + (size_t)qcap * (8 + 4 + 2) + 16;
#define MPREID_JACCARD_LAUNCH(JT_, NPF_, PD_, PK_)                                                                       \
    {                                                                                                                    \
        int rc = mpreid_dyn_lds(jaccard_kernel<JT_, NPF_, PD_, PK_>, lds);                                                  \
        if (rc) return rc;                                                                                               \
        hipLaunchKernelGGL((jaccard_kernel<JT_, NPF_, PD_, PK_>), dim3((unsigned)qrows, (unsigned)nchunks), dim3(JT_),   \
                           lds, stream, N, nq, MT, ld, rowmax, fcnt, fidx, fval, qcap, cptr, crow, cval, rch, oml, lam32, \
                           out, ldo, pair_counter, q0, Hp, rpb, bpc, jdbg);                                              \
    }
    // (multi-wave form, N = 20 000 / Market shape: 512 threads <2, 4> 1.58 / 1.42 ms, 256 threads <3, 4> 1.36 / 1.21,
    // <3, 8> the same, <2, 4> 2.05 (columns longer than 512 entries take the direct path), 128 threads <5, 4> 1.72 / 1.50)
    // blocked index = packed entries (csc2_fill_kernel); the atomic build keeps (row, value) in two arrays
    static const int jtab = mpreid_tune("jaccard_table", 0);   // A/B: LDS table form
    const size_t wl = align_up((size_t)rch * 2 + 16, 16);   // table-free kernels: the accumulators only
    if (threads == 64 && !jtab) {
        int rc = mpreid_dyn_lds(jaccard_wave_kernel<64, 2, 8>, wl);
        if (rc) return rc;
        hipLaunchKernelGGL((jaccard_wave_kernel<64, 2, 8>), dim3((unsigned)qrows, (unsigned)nchunks), dim3(64), wl, stream, N, nq,
                           MT, ld, rowmax, fcnt, fidx, fval, qcap, cptr, (const unsigned *)crow, rch, oml, lam32, out, ldo,
                           pair_counter, q0, Hp, rpb, bpc);
    } else if (threads == 64) MPREID_JACCARD_LAUNCH(64, 2, 8, true)
    else if (blocked && !jtab) {
        int rc = mpreid_dyn_lds(jaccard_wave_kernel<JT, 3, 4>, wl);
        if (rc) return rc;
        hipLaunchKernelGGL((jaccard_wave_kernel<JT, 3, 4>), dim3((unsigned)qrows, (unsigned)nchunks), dim3(JT), wl, stream, N, nq,
                           MT, ld, rowmax, fcnt, fidx, fval, qcap, cptr, (const unsigned *)crow, rch, oml, lam32, out, ldo,
                           pair_counter, q0, Hp, rpb, bpc);
    }
    else if (blocked) MPREID_JACCARD_LAUNCH(JT, 3, 4, true)
    else MPREID_JACCARD_LAUNCH(JT, 3, 4, false)
#undef MPREID_JACCARD_LAUNCH
    LAUNCH_CHECK();
    return MPREID_OK;
}

// mpreid_rerank_stats from the counters ([0] Jaccard pairs .. [6] nnz(V_qe)), the caps, the algorithm and the stage marks:
// marks 0..3 are start / distances / neighbours / V rows in every algorithm; the expansion runs from mark qe0 to mark csc0,
// less the in-line distance rows of the queries between the marks dq0 and dq1 (dq0 == dq1: none; timed_dq: reported as
// ms_dq); the index build and the Jaccard stage take one mark each after csc0
void fill_rerank_stats(mpreid_rerank_stats *stats, int64_t N, int k1, int k2, int h, int vcap, int vqe_cap,
                       const unsigned long long cnt[7], int algo, StageTimer &tm, int qe0, int dq0, int dq1, int csc0,
                       bool timed_dq) {
    if (!stats) return;
    stats->n = N; stats->k1 = k1; stats->k2 = k2; stats->half_k1 = h; stats->v_cap = vcap; stats->vqe_cap = vqe_cap;
    stats->v_nnz = (int64_t)cnt[2];
    stats->vqe_nnz = (int64_t)cnt[6];   // (all rows; the inverted index holds the gallery rows only)
    stats->jaccard_pairs = (int64_t)cnt[0];
    stats->krecip_r_sum = (int64_t)cnt[1];
    stats->fallback_rows = (int64_t)(cnt[4] & 0xffffffffull);   // (these two: zero unless the sparse algorithm ran)
    stats->cand_total = (int64_t)cnt[5];
    stats->algo = algo;
    stats->ms_gemm = tm.ms(0, 1); stats->ms_topk = tm.ms(1, 2); stats->ms_krecip = tm.ms(2, 3);
    stats->ms_dq = timed_dq ? tm.ms(dq0, dq1) : 0.0f;   // (side stream: filled in by the caller)
    stats->ms_qe = dq1 != dq0 ? tm.ms(qe0, dq0) + tm.ms(dq1, csc0) : tm.ms(qe0, csc0);
    stats->ms_csc = tm.ms(csc0, csc0 + 1); stats->ms_jaccard = tm.ms(csc0 + 1, csc0 + 2); stats->ms_total = tm.ms(0, csc0 + 2);
}

int rerank_tail(const TailArgs &a, hipStream_t stream, StageTimer &tm, mpreid_rerank_stats *stats, int marks_so_far) {
    const int64_t N = a.N;
    const int k2e = (int)std::min<int64_t>(a.k2, N); // rows the query expansion really averages (numpy clamps the slice)
    int qcap = a.vcap;
    const int *fcnt = a.vcnt, *fidx = a.vidx;
    const uint16_t *fval = a.vval;
    bool mid_done = false;
    // (7) query expansion
    launch_sum_i32(a.vcnt, N, a.counters + 2, stream);
    if (a.k2 != 1) {
        {
            int rc = launch_qe_count(N, a.rank, a.KR, k2e, 0, N, a.vcnt, a.vidx, a.vcap, a.ucnt, stream);
            if (rc) return rc;
            launch_max_i32(a.ucnt, N, (int *)(a.counters + 3), stream);
            LAUNCH_CHECK();
        }
        int mxu = 1;
        HIP_TRY(hipMemcpyAsync(&mxu, a.counters + 3, 4, hipMemcpyDeviceToHost, stream));
        tm.mark(); // +1
        if (a.mid_launch && a.sized) {
            HIP_TRY(hipEventRecord(a.sized, stream));
            int rc = a.mid_launch(stream);
            if (rc) return rc;
            tm.mark(); // +2
            HIP_TRY(hipEventSynchronize(a.sized));
        } else {
            tm.mark(); // +2
            HIP_TRY(hipStreamSynchronize(stream));
        }
        mid_done = true;
        if (mxu < 1) mxu = 1;
        qcap = (int)align_up((size_t)mxu, 8);
        if ((int64_t)qcap > a.qcap_bound) {
            if ((int64_t)mxu <= a.qcap_bound) {
                qcap = (int)a.qcap_bound;
            } else {
                mpreid_set_error("query expansion: a row has %d entries, the workspace was sized for %lld; retry with "
                                 "MPREID_RERANK_DENSE", mxu, (long long)a.qcap_bound);
                return MPREID_ERR_RETRY_DENSE;
            }
        }
        {
            int rc = launch_qe_fill(N, a.rank, a.KR, k2e, 0, N, a.vcnt, a.vidx, a.vval, a.vcap, qcap, a.qcnt, a.qidx, a.qval,
                                    stream);
            if (rc) return rc;
        }
        fcnt = a.qcnt;
        fidx = a.qidx;
        fval = a.qval;
    }
    if (!mid_done) {   // k2 == 1: no expansion, no sizing
        tm.mark(); // +1
        if (a.mid_launch) {
            int rc = a.mid_launch(stream);
            if (rc) return rc;
        }
        tm.mark(); // +2
    }
    launch_sum_i32(fcnt, N, a.counters + 6, stream);   // nnz(V_qe), all rows
    tm.mark(); // +3
    // inverted index
    bool blocked_csc = false;
    {
        int rc = launch_csc(N, a.nq, fcnt, fidx, fval, qcap, a.ccnt, a.chist, a.cptr, a.crow, a.cval, stream, &blocked_csc);
        if (rc) return rc;
    }
    tm.mark(); // +4
    // (8)-(11) Jaccard + blend
    if (a.join) HIP_TRY(hipStreamWaitEvent(stream, a.join, 0));
    {
        int rc = launch_jaccard(N, a.nq, 0, a.nq, a.MT, a.ld, a.rowmax, fcnt, fidx, fval, qcap, a.cptr, a.crow, a.cval, a.chist,
                                blocked_csc, a.lambda_value, a.out, a.ldo, a.counters, stream);
        if (rc) return rc;
    }
    tm.mark(); // +5
    unsigned long long cnt[7] = {0, 0, 0, 0, 0, 0, 0};
    long long nnz_total = 0;
    HIP_TRY(hipMemcpyAsync(cnt, a.counters, sizeof(cnt), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(&nnz_total, a.cptr + N, 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    const int m = marks_so_far;   // index of the mark taken after the V rows
    fill_rerank_stats(stats, N, a.k1, a.k2, a.h, a.vcap, qcap, cnt, a.algo, tm, m, m + 1, m + 2, m + 3, (bool)a.mid_launch);
    return MPREID_OK;
}

static int rerank_dense(const float *q, const float *g, int64_t nq, int64_t ng, int d, int k1, int k2,
                                 double lambda_value, const float *local, int only_local, float *out, int64_t ldo,
                                 void *ws, size_t ws_bytes, mpreid_stream_t stream_, mpreid_rerank_stats *stats,
                                 int timing) {
    ARG_CHECK(q && g && out && nq > 0 && ng > 0 && d > 0 && k1 >= 0 && k2 >= 1 && ldo >= ng);
    ARG_CHECK(!only_local || local);
    const RerankLayout L = make_layout(nq, ng, d, k1, k2, local != nullptr);
    const int64_t N = L.N;
    ARG_CHECK(L.KR <= N);
    if (!dense_kr_ok(L)) {
        mpreid_set_error("re_ranking: max(k1 + 1, k2) = %d exceeds this build's limit of 256 (the neighbour selection sorts its "
                         "winners in one 256-entry LDS network and the reciprocity masks hold 256 bits per row; include/mpreid.h). "
                         "The reference (utils/reranking.py:29) takes any k and is called with k1 = 50, k2 = 15", L.KR);
        return MPREID_ERR_UNSUPPORTED;
    }
    if (N >= (1ll << 31) - 64) {
        mpreid_set_error("N too large");
        return MPREID_ERR_UNSUPPORTED;
    }
    if (!ws || ws_bytes < L.total) {
        mpreid_set_error("rerank workspace too small: %zu < %zu", ws_bytes, L.total);
        return MPREID_ERR_WORKSPACE;
    }
    hipStream_t stream = (hipStream_t)stream_;
    char *base = (char *)ws;
    float *feat = (float *)(base + L.feat), *norms = (float *)(base + L.norms);
    float *D = (float *)(base + L.D), *MT = (float *)(base + L.MT), *rowmax = (float *)(base + L.rowmax);
    int *rank = (int *)(base + L.rank), *vcnt = (int *)(base + L.vcnt), *vidx = (int *)(base + L.vidx);
    uint16_t *vval = (uint16_t *)(base + L.vval);
    int *ucnt = (int *)(base + L.ucnt), *qcnt = (int *)(base + L.qcnt), *qidx = (int *)(base + L.qidx);
    uint16_t *qval = (uint16_t *)(base + L.qval);
    unsigned *ccnt = (unsigned *)(base + L.ccnt);
    long long *cptr = (long long *)(base + L.cptr);
    int *crow = (int *)(base + L.crow);
    uint16_t *cval = (uint16_t *)(base + L.cval);
    unsigned long long *counters = (unsigned long long *)(base + L.counters);

    StageTimer tm(timing != 0, stream);
    HIP_TRY(hipMemsetAsync(counters, 0, 64, stream));
    tm.mark(); // 0
    {   // (1) original_dist
        int rc = launch_original_dist(q, g, nq, ng, d, local, only_local, feat, norms, D, MT, L.ld, stream);
        if (rc) return rc;
    }
    tm.mark(); // 1
    // (2)+(3) row max and the first KR neighbours in (value, index) order
    {
        int rc = launch_rowmax_topk(MT, L.ld, N, L.KR, N, rowmax, rank, stream);
        if (rc) return rc;
    }
    tm.mark(); // 2
    // (4)-(6) V rows
    {
        int rc = launch_krecip(false, MT, L.ld, N, rowmax, rank, L.K, L.KR, L.h, L.vcap, vcnt, vidx, vval, 0, N, ucnt, nullptr,
                               nullptr, 0, nullptr, (unsigned *)(base + L.rbits), stream);
        if (rc) return rc;
        launch_sum_i32(ucnt, N, counters + 1, stream);
        LAUNCH_CHECK();
    }
    tm.mark(); // 3
    TailArgs ta{};
    ta.N = N; ta.nq = nq; ta.k1 = k1; ta.k2 = k2; ta.KR = L.KR; ta.h = L.h; ta.vcap = L.vcap; ta.qcap_bound = L.qcap_bound;
    ta.rank = rank; ta.vcnt = vcnt; ta.vidx = vidx; ta.vval = vval; ta.ucnt = ucnt; ta.qcnt = qcnt; ta.qidx = qidx;
    ta.qval = qval; ta.ccnt = ccnt; ta.cptr = cptr; ta.crow = crow; ta.cval = cval; ta.counters = counters;
    ta.chist = (unsigned *)(base + L.chist);
    ta.MT = MT; ta.ld = L.ld; ta.rowmax = rowmax; ta.out = out; ta.ldo = ldo; ta.lambda_value = lambda_value;
    ta.algo = MPREID_RERANK_DENSE;
    return rerank_tail(ta, stream, tm, stats, 3);
}

// Would `algo` accept this problem?  1 / 0; no side effects, no device needed.  The two documented limits of DENSE (and
// of AUTO when SPARSE does not apply) are evaluated with the expressions the launchers use.
extern "C" int mpreid_rerank_fits(int64_t nq, int64_t ng, int d, int k1, int k2, int has_local, int algo) {
    if (nq <= 0 || ng <= 0 || d <= 0 || k1 < 0 || k2 < 1 || nq + ng >= (1ll << 31) - 64) return 0;
    if (algo == MPREID_RERANK_WIDE) return wide_fits(nq, ng) ? 1 : 0;
    const bool eligible = sparse_eligible(nq, ng, k1, k2, has_local ? (const float *)1 : nullptr);
    if (algo == MPREID_RERANK_SPARSE || algo == MPREID_RERANK_SPARSE_SPLIT3) return eligible ? 1 : 0;
    if (algo == MPREID_RERANK_AUTO && eligible) return 1;
    if (algo != MPREID_RERANK_AUTO && algo != MPREID_RERANK_DENSE) return 0;
    const RerankLayout L = make_layout(nq, ng, d, k1, k2, has_local);
    return (dense_kr_ok(L) && dense_lds_ok(L)) ? 1 : 0;
}

extern "C" size_t mpreid_rerank_workspace_bytes_ex(int64_t nq, int64_t ng, int d, int k1, int k2, int has_local, int algo) {
    if (nq < 0 || ng < 0 || d <= 0 || k1 < 0 || k2 < 1) return 0;
    if (algo == MPREID_RERANK_WIDE) return make_layout_wide(nq, ng, d, k1, k2, has_local).total;
    const bool sparse = algo == MPREID_RERANK_SPARSE || algo == MPREID_RERANK_SPARSE_SPLIT3 ||
                        (algo == MPREID_RERANK_AUTO && sparse_eligible(nq, ng, k1, k2, has_local ? (const float *)1 : nullptr));
    return sparse ? make_layout2(nq, ng, d, k1, k2, algo == MPREID_RERANK_SPARSE_SPLIT3).total
                  : make_layout(nq, ng, d, k1, k2, has_local).total;
}
// The plain pair (mpreid_rerank_workspace_bytes + mpreid_rerank_f32: the binding INTEGRATION.md shows) is the DENSE
// algorithm: any N, local_distmat supported, no data-dependent MPREID_ERR_RETRY_DENSE -- it never fails on data.  The
// faster sparse algorithm (and the retry protocol that goes with it) is opt-in through the _ex entry points.
extern "C" size_t mpreid_rerank_workspace_bytes(int64_t nq, int64_t ng, int d, int k1, int k2, int has_local) {
    return mpreid_rerank_workspace_bytes_ex(nq, ng, d, k1, k2, has_local, MPREID_RERANK_DENSE);
}

extern "C" int mpreid_rerank_f32_ex(const float *q, const float *g, int64_t nq, int64_t ng, int d, int k1, int k2,
                                    double lambda_value, const float *local, int only_local, float *out, int64_t ldo,
                                    void *ws, size_t ws_bytes, mpreid_stream_t stream, mpreid_rerank_stats *stats,
                                    int timing, int algo) {
    ARG_CHECK(algo == MPREID_RERANK_AUTO || algo == MPREID_RERANK_DENSE || algo == MPREID_RERANK_SPARSE ||
              algo == MPREID_RERANK_SPARSE_SPLIT3 || algo == MPREID_RERANK_WIDE);
    if (algo == MPREID_RERANK_WIDE)
        return rerank_wide(q, g, nq, ng, d, k1, k2, lambda_value, local, only_local, out, ldo, ws, ws_bytes, stream, stats,
                           timing);
    const bool eligible = sparse_eligible(nq, ng, k1, k2, local);
    const bool want_sparse = algo == MPREID_RERANK_SPARSE || algo == MPREID_RERANK_SPARSE_SPLIT3;
    if (want_sparse && !eligible) {
        mpreid_set_error("the sparse re-ranking algorithm needs N >= 2048, max(k1+1, k2) <= 64 and no local_distmat");
        return MPREID_ERR_UNSUPPORTED;
    }
    if (want_sparse || (algo == MPREID_RERANK_AUTO && eligible))
        return rerank_sparse(q, g, nq, ng, d, k1, k2, lambda_value, out, ldo, ws, ws_bytes, stream, stats, timing,
                             algo == MPREID_RERANK_SPARSE_SPLIT3);
    return rerank_dense(q, g, nq, ng, d, k1, k2, lambda_value, local, only_local, out, ldo, ws, ws_bytes, stream, stats,
                        timing);
}
extern "C" int mpreid_rerank_f32(const float *q, const float *g, int64_t nq, int64_t ng, int d, int k1, int k2,
                                 double lambda_value, const float *local, int only_local, float *out, int64_t ldo,
                                 void *ws, size_t ws_bytes, mpreid_stream_t stream, mpreid_rerank_stats *stats,
                                 int timing) {
    return mpreid_rerank_f32_ex(q, g, nq, ng, d, k1, k2, lambda_value, local, only_local, out, ldo, ws, ws_bytes, stream,
                                stats, timing, MPREID_RERANK_DENSE);
}

extern "C" int mpreid_rerank_debug_copy(const void *ws, int64_t nq, int64_t ng, int d, int k1, int k2, int has_local,
                                        int32_t *rank_out, int32_t *v_cnt, int32_t *vqe_cnt,
                                        mpreid_stream_t stream_) {
    return mpreid_rerank_debug_copy_ex(ws, nq, ng, d, k1, k2, has_local, rank_out, v_cnt, vqe_cnt, stream_,
                                       MPREID_RERANK_DENSE);
}

extern "C" int mpreid_rerank_debug_copy_ex(const void *ws, int64_t nq, int64_t ng, int d, int k1, int k2, int has_local,
                                           int32_t *rank_out, int32_t *v_cnt, int32_t *vqe_cnt,
                                           mpreid_stream_t stream_, int algo) {
    ARG_CHECK(ws && (algo == MPREID_RERANK_DENSE || algo == MPREID_RERANK_SPARSE || algo == MPREID_RERANK_SPARSE_SPLIT3 ||
                     algo == MPREID_RERANK_WIDE));
    // the fields the taps read, from whichever layout the call used
    struct { int64_t N; int K, KR; size_t rank, vcnt, qcnt; } L;
    if (algo == MPREID_RERANK_WIDE) {
        const WideLayout s3 = make_layout_wide(nq, ng, d, k1, k2, has_local);
        L.N = s3.N; L.K = s3.K; L.KR = s3.KR; L.rank = s3.rank; L.vcnt = s3.vcnt; L.qcnt = s3.qcnt;
    } else if (algo != MPREID_RERANK_DENSE) {
        const Rerank2Layout s2 = make_layout2(nq, ng, d, k1, k2);
        L.N = s2.N; L.K = s2.K; L.KR = s2.KR; L.rank = s2.rank; L.vcnt = s2.vcnt; L.qcnt = s2.qcnt;
    } else {
        const RerankLayout s1 = make_layout(nq, ng, d, k1, k2, has_local);
        L.N = s1.N; L.K = s1.K; L.KR = s1.KR; L.rank = s1.rank; L.vcnt = s1.vcnt; L.qcnt = s1.qcnt;
    }
    hipStream_t stream = (hipStream_t)stream_;
    const char *base = (const char *)ws;
    if (rank_out) { // [N][k1+1]; columns past min(k1+1, N) are -1
        for (int64_t t = 0; t < L.N * (int64_t)(k1 + 1); ++t) rank_out[t] = -1;
        HIP_TRY(hipMemcpy2DAsync(rank_out, (size_t)(k1 + 1) * 4, base + L.rank, (size_t)L.KR * 4, (size_t)L.K * 4,
                                 (size_t)L.N, hipMemcpyDeviceToHost, stream));
    }
    if (v_cnt) HIP_TRY(hipMemcpyAsync(v_cnt, base + L.vcnt, (size_t)L.N * 4, hipMemcpyDeviceToHost, stream));
    if (vqe_cnt)
        HIP_TRY(hipMemcpyAsync(vqe_cnt, base + (k2 != 1 ? L.qcnt : L.vcnt), (size_t)L.N * 4, hipMemcpyDeviceToHost,
                               stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return MPREID_OK;
}

// ---------------------------------------------------------------------------------------------
// Row-sharded re-ranking (every mpreid_rr_* entry point and the CSR transport of the sparse rows): the
// launchers of this file and of the other rerank_*.hip files driven phase by phase over a row range
// [r_lo, r_lo + rows) of the N x N problem.  Between the phases the caller all-gathers the rank table, the
// sparse V rows and the sparse V_qe rows (mpreid/distributed.py: RCCL through torch.distributed).  No
// floating-point reduction crosses ranks and every row is computed by exactly the same instruction
// sequence as on one GPU, so the result does not depend on the number of ranks.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rowmax_kernel(const float *__restrict__ M, int64_t ld, int64_t N,
                                                     float *__restrict__ rowmax) {
    __shared__ float s_red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *row = M + (int64_t)blockIdx.x * ld;
    float mx = -3.402823466e+38f;
    for (int j = tid; j < (int)N; j += 256) mx = fmaxf(mx, row[j]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
    if (lane == 0) s_red[wave] = mx;
    __syncthreads();
    if (tid == 0) rowmax[blockIdx.x] = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
}

// copy ELL rows from row stride `ss` to row stride `ds` (ds >= max count); entries past the count are zeroed
__global__ __launch_bounds__(256) void pack_rows_kernel(const int *__restrict__ cnt, const int *__restrict__ idx,
                                                        const uint16_t *__restrict__ val, int64_t rows, int ss, int ds,
                                                        int *__restrict__ idx_out, uint16_t *__restrict__ val_out) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int c = cnt[r];
    for (int a = lane; a < ds; a += 64) {
        idx_out[r * ds + a] = a < c ? idx[r * ss + a] : 0;
        val_out[r * ds + a] = a < c ? val[r * ss + a] : (uint16_t)0;
    }
}

// phase 1: rows [r_lo, r_lo+rows) of D = |f_i|^2 + |f_j|^2 - 2 f_i.f_j  (norms_all from mpreid_sqnorm_f32),
// their row maxima and (if rank_local != NULL) their first KR neighbours.  D_local [rows][ld], ld >= N.
extern "C" int mpreid_rr_dist_rows(const float *feat_all, const float *norms_all, int64_t n, int d, int64_t r_lo,
                                   int64_t rows, float *d_local, int64_t ld, float *rowmax_local, int32_t *rank_local,
                                   int kr, mpreid_stream_t stream_) {
    ARG_CHECK(feat_all && norms_all && d_local && rowmax_local && n > 0 && d > 0 && rows > 0 && r_lo >= 0 &&
              r_lo + rows <= n && ld >= n);
    hipStream_t stream = (hipStream_t)stream_;
    int rc = mpreid_distance_launch(feat_all + r_lo * (int64_t)d, feat_all, rows, n, d, norms_all + r_lo, norms_all,
                                    d_local, ld, 0, stream);
    if (rc) return rc;
    if (rank_local) {
        ARG_CHECK(kr >= 1 && kr <= 256 && kr <= n);
        rc = launch_rowmax_topk(d_local, ld, n, kr, rows, rowmax_local, rank_local, stream);
        if (rc) return rc;
    } else {
        hipLaunchKernelGGL(rowmax_kernel, dim3((unsigned)rows), dim3(256), 0, stream, d_local, ld, n, rowmax_local);
    }
    LAUNCH_CHECK();
    return MPREID_OK;
}

// phase 2: V rows of the local row range from the GLOBAL rank table; ELL with row stride vcap =
// min(N, (k1+1)*(1+half_k1)) (mpreid_rr_vcap)
extern "C" int mpreid_rr_vcap(int64_t n, int k1) { return clamp_k(n, k1, 1).vcap; }

extern "C" size_t mpreid_rr_krecip_scratch_bytes(int64_t n) { return (size_t)n * RB_WORDS * 4 * 2; }

extern "C" int mpreid_rr_krecip(const float *d_local, int64_t ld, int64_t n, const float *rowmax_local,
                                const int32_t *rank_all, int k1, int kr, int64_t r_lo, int64_t rows, int32_t *vcnt,
                                int32_t *vidx, uint16_t *vval, void *scratch, mpreid_stream_t stream_) {
    const RerankK k = clamp_k(n, k1, 1);   // (the table width kr is the caller's)
    ARG_CHECK(d_local && rowmax_local && rank_all && vcnt && vidx && vval && scratch && rows > 0 && kr >= k.K);
    // reciprocity bits of ALL rows (candidates of a local row live anywhere): recomputed by every rank from the
    // all-gathered table -- N x K membership tests, cheaper than another exchange
    return launch_krecip(false, d_local, ld, n, rowmax_local, rank_all, k.K, kr, k.h, k.vcap, vcnt, vidx, vval, r_lo, rows, nullptr,
                         nullptr, nullptr, 0, nullptr, (unsigned *)scratch, (hipStream_t)stream_);
}

// ---------------------------------------------------------------------------------------------
// Row-sharded SPARSE phases (the multi-GPU form of the candidate pipeline): a rank's rows [r_lo, r_lo + rows) of the
// N x N problem without its [rows][N] distance block.
//   mpreid_rr_neighbours_sparse   phase 1: fp16 operands of all rows (every rank needs all columns), sample pass and
//                                 thresholds for the local rows, candidate GEMM local rows x all columns (no symmetry
//                                 to exploit inside a row block), exact refinement + fallback rows
//                                 -> rank_local [rows][kr], rowmax_local [rows], rankd_local [rows][kr]
//   mpreid_rr_krecip_sparse       phase 2 with on-the-fly exact distances (no D rows)
// Phases 3 and 4 are the existing ones (the Jaccard phase computes the exact rows of the LOCAL QUERIES only).  Same
// bits as the dense phases and the single-GPU call.  MPREID_ERR_RETRY_DENSE: use mpreid_rr_dist_rows for this rank.
// ---------------------------------------------------------------------------------------------
// workspace of phase 1: the candidate buffers alone, the operands with RR_SLACK rows of slack (the local row block is read
// in whole 256-row tiles)
constexpr int64_t RR_SLACK = 256;
extern "C" size_t mpreid_rr_sparse_workspace_bytes(int64_t n, int d, int64_t rows, int kr) {
    if (n <= 0 || d <= 0 || rows <= 0 || kr <= 0) return 0;
    WsCursor take;
    (void)take_cand_buffers(take, n, d, rows, kr, RR_SLACK);
    return take.off;
}

extern "C" int mpreid_rr_neighbours_sparse(const float *feat_all, const float *norms_all, int64_t n, int d, int64_t r_lo,
                                           int64_t rows, int kr, int32_t *rank_local, float *rowmax_local, float *rankd_local,
                                           void *ws, size_t ws_bytes, mpreid_stream_t stream_) {
    ARG_CHECK(feat_all && norms_all && rank_local && rowmax_local && rankd_local && n >= 2048 && d > 0 && rows > 0 && r_lo >= 0 &&
              r_lo + rows <= n && kr >= 1 && kr <= 64 && kr <= n);
    WsCursor take;
    const CandBuffers c = take_cand_buffers(take, n, d, rows, kr, RR_SLACK);
    if (!ws || ws_bytes < take.off) {
        mpreid_set_error("sparse phase-1 workspace too small: %zu < %zu", ws_bytes, take.off);
        return MPREID_ERR_WORKSPACE;
    }
    hipStream_t stream = (hipStream_t)stream_;
    char *base = (char *)ws;
    float *sqn = (float *)(base + c.sqn), *gstat = (float *)(base + c.gstat);
    unsigned *fb_count = (unsigned *)(base + c.fb_count);

    HIP_TRY(hipMemsetAsync(fb_count, 0, 64, stream));
    HIP_TRY(hipMemsetAsync(rank_local, 0, (size_t)rows * kr * 4, stream));
    HIP_TRY(hipMemsetAsync(rankd_local, 0, (size_t)rows * kr * 4, stream));
    HIP_TRY(hipMemsetAsync(rowmax_local, 0, (size_t)rows * 4, stream));
    HIP_TRY(hipMemsetAsync(sqn, 0, (size_t)(c.Np + c.slack) * 4, stream));
    HIP_TRY(hipMemcpyAsync(sqn, norms_all, (size_t)n * 4, hipMemcpyDeviceToDevice, stream));
    int rc = cand_lists(feat_all, base, c, n, d, r_lo, rows, 0, 0, stream);
    if (rc) return rc;
    rc = cand_refine(feat_all, base, c, n, d, kr, r_lo, rows, rowmax_local, rank_local, rankd_local, stream);
    if (rc) return rc;
    float gs[2] = {0.f, 0.f};
    unsigned fbc = 0;
    HIP_TRY(hipMemcpyAsync(gs, gstat, 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(&fbc, fb_count, 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (gs[1] != 0.0f || fbc > (unsigned)c.fb_max) {
        mpreid_set_error("sparse phase 1: %s; use mpreid_rr_dist_rows for this row block",
                         gs[1] != 0.0f ? "row norms too large for fp16 operands" : "too many rows needed the dense fallback");
        return MPREID_ERR_RETRY_DENSE;
    }
    return MPREID_OK;
}

extern "C" int mpreid_rr_krecip_sparse(const float *feat_all, const float *norms_all, int64_t n, int d,
                                       const float *rowmax_local, const int32_t *rank_all, const float *rankd_local, int k1,
                                       int kr, int64_t r_lo, int64_t rows, int32_t *vcnt, int32_t *vidx, uint16_t *vval,
                                       void *scratch, mpreid_stream_t stream_) {
    const RerankK k = clamp_k(n, k1, 1);
    ARG_CHECK(feat_all && norms_all && rowmax_local && rank_all && rankd_local && vcnt && vidx && vval && scratch && rows > 0 &&
              kr >= k.K);
    // rankd is indexed by the global row inside the kernel: shift the local table's base accordingly
    return launch_krecip(true, nullptr, 0, n, rowmax_local, rank_all, k.K, kr, k.h, k.vcap, vcnt, vidx, vval, r_lo, rows, nullptr,
                         feat_all, norms_all, d, rankd_local - (int64_t)r_lo * kr, (unsigned *)scratch, (hipStream_t)stream_);
}

extern "C" int mpreid_rr_pack_rows(const int32_t *cnt, const int32_t *idx, const uint16_t *val, int64_t rows,
                                   int src_stride, int dst_stride, int32_t *idx_out, uint16_t *val_out,
                                   mpreid_stream_t stream_) {
    ARG_CHECK(cnt && idx && val && idx_out && val_out && rows > 0 && src_stride > 0 && dst_stride > 0);
    hipLaunchKernelGGL(pack_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream_, cnt, idx,
                       val, rows, src_stride, dst_stride, idx_out, val_out);
    LAUNCH_CHECK();
    return MPREID_OK;
}

// ---- CSR transport of the sparse rows (the all-gathers of V and V_qe move nnz entries instead of rows x global max) ----
// rowptr[0 .. rows] = exclusive prefix sums of cnt (one workgroup walks the rows in 1024-row chunks with a running carry)
__global__ __launch_bounds__(1024) void rowptr_scan_kernel(const int *__restrict__ cnt, int64_t rows, long long *__restrict__ rowptr) {
    __shared__ long long wsum[16];
    __shared__ long long carry_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) carry_s = 0;
    __syncthreads();
    for (int64_t base = 0; base < rows; base += 1024) {
        const int64_t i = base + tid;
        const long long v = i < rows ? (long long)cnt[i] : 0;
        long long x = v;   // inclusive scan inside the wave
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const long long y = __shfl_up(x, off, 64);
            if (lane >= off) x += y;
        }
        if (lane == 63) wsum[wave] = x;
        __syncthreads();
        long long pre = carry_s;
        for (int w = 0; w < wave; ++w) pre += wsum[w];
        if (i < rows) rowptr[i] = pre + x - v;
        __syncthreads();
        if (tid == 1023) carry_s = pre + x;
        __syncthreads();
    }
    if (tid == 0) rowptr[rows] = carry_s;
}

// TO_CSR: packed[rowptr[r] + e] = ell[r][e] for e < cnt[r]; else the inverse (ELL padding is left untouched)
template <bool TO_CSR>
__global__ __launch_bounds__(256) void csr_ell_kernel(const long long *__restrict__ rowptr, int64_t rows, int stride,
                                                      int *__restrict__ ell_idx, uint16_t *__restrict__ ell_val,
                                                      int *__restrict__ csr_idx, uint16_t *__restrict__ csr_val) {
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const long long p0 = rowptr[r];
    const int n = (int)(rowptr[r + 1] - p0);
    for (int e = threadIdx.x & 63; e < n; e += 64) {
        if (TO_CSR) {
            csr_idx[p0 + e] = ell_idx[r * stride + e];
            csr_val[p0 + e] = ell_val[r * stride + e];
        } else {
            ell_idx[r * stride + e] = csr_idx[p0 + e];
            ell_val[r * stride + e] = csr_val[p0 + e];
        }
    }
}

extern "C" int mpreid_rr_rowptr(const int32_t *cnt, int64_t rows, long long *rowptr, mpreid_stream_t stream_) {
    ARG_CHECK(cnt && rowptr && rows >= 0);
    hipLaunchKernelGGL(rowptr_scan_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream_, cnt, rows, rowptr);
    LAUNCH_CHECK();
    return MPREID_OK;
}

extern "C" int mpreid_rr_ell_to_csr(const long long *rowptr, const int32_t *idx, const uint16_t *val, int64_t rows, int stride,
                                    int32_t *idx_out, uint16_t *val_out, mpreid_stream_t stream_) {
    ARG_CHECK(rowptr && idx && val && idx_out && val_out && rows >= 0 && stride > 0);
    if (rows == 0) return MPREID_OK;
    hipLaunchKernelGGL(csr_ell_kernel<true>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream_, rowptr, rows,
                       stride, const_cast<int *>(idx), const_cast<uint16_t *>(val), idx_out, val_out);
    LAUNCH_CHECK();
    return MPREID_OK;
}

extern "C" int mpreid_rr_csr_to_ell(const long long *rowptr, const int32_t *idx, const uint16_t *val, int64_t rows, int stride,
                                    int32_t *idx_out, uint16_t *val_out, mpreid_stream_t stream_) {
    ARG_CHECK(rowptr && idx && val && idx_out && val_out && rows >= 0 && stride > 0);
    if (rows == 0) return MPREID_OK;
    hipLaunchKernelGGL(csr_ell_kernel<false>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream_, rowptr, rows,
                       stride, idx_out, val_out, const_cast<int *>(idx), const_cast<uint16_t *>(val));
    LAUNCH_CHECK();
    return MPREID_OK;
}

// phase 3: query expansion of the local rows from the GLOBAL V (row stride vstride).  Two steps: union sizes
// (ucnt_local), then the fill with row stride qcap >= max union size.
extern "C" int mpreid_rr_qe_count(int64_t n, const int32_t *rank_all, int kr, int k2, int64_t r_lo, int64_t rows,
                                  const int32_t *vcnt_all, const int32_t *vidx_all, int vstride, int32_t *ucnt_local,
                                  mpreid_stream_t stream_) {
    ARG_CHECK(rank_all && vcnt_all && vidx_all && ucnt_local && rows > 0 && k2 >= 1 && kr >= k2);
    return launch_qe_count(n, rank_all, kr, k2, r_lo, rows, vcnt_all, vidx_all, vstride, ucnt_local, (hipStream_t)stream_);
}

extern "C" int mpreid_rr_qe_fill(int64_t n, const int32_t *rank_all, int kr, int k2, int64_t r_lo, int64_t rows,
                                 const int32_t *vcnt_all, const int32_t *vidx_all, const uint16_t *vval_all, int vstride,
                                 int qcap, int32_t *qcnt_local, int32_t *qidx_local, uint16_t *qval_local,
                                 mpreid_stream_t stream_) {
    ARG_CHECK(rank_all && vcnt_all && vidx_all && vval_all && qcnt_local && qidx_local && qval_local && rows > 0 &&
              qcap > 0);
    return launch_qe_fill(n, rank_all, kr, k2, r_lo, rows, vcnt_all, vidx_all, vval_all, vstride, qcap, qcnt_local, qidx_local,
                          qval_local, (hipStream_t)stream_);
}

// phase 4: inverted index of the GLOBAL V_qe (row stride qstride) + Jaccard / blend for the query rows
// [q_lo, q_lo + qrows): d_q [qrows][ld] and rowmax_q from mpreid_rr_dist_rows on that range.
// Scratch: ccnt [N+1] u32, cptr [N+1] i64, crow [nnz] i32, cval [nnz] u16 (nnz = sum of qcnt_all).
extern "C" size_t mpreid_rr_jaccard_hist_bytes(int64_t n) { return csc_hist_bytes(n); }

extern "C" int mpreid_rr_jaccard(int64_t n, int64_t nq, int64_t q_lo, int64_t qrows, const float *d_q, int64_t ld,
                                 const float *rowmax_q, const int32_t *qcnt_all, const int32_t *qidx_all,
                                 const uint16_t *qval_all, int qstride, double lambda_value, uint32_t *ccnt,
                                 long long *cptr, int32_t *crow, uint16_t *cval, uint32_t *chist, float *out, int64_t ldo,
                                 mpreid_stream_t stream_) {
    ARG_CHECK(d_q && rowmax_q && qcnt_all && qidx_all && qval_all && ccnt && cptr && crow && cval && out && qrows > 0 &&
              q_lo >= 0 && q_lo + qrows <= nq && ldo >= n - nq);
    hipStream_t stream = (hipStream_t)stream_;
    bool blocked = false;
    int rc = launch_csc(n, nq, qcnt_all, qidx_all, qval_all, qstride, ccnt, chist, cptr, crow, cval, stream, &blocked);
    if (rc) return rc;
    return launch_jaccard(n, nq, (int)q_lo, qrows, d_q, ld, rowmax_q, qcnt_all, qidx_all, qval_all, qstride, cptr, crow, cval,
                          chist, blocked, lambda_value, out, ldo, nullptr, stream);
}

// ---- column-sharded build of the inverted index (phase 4 of the row-sharded re-ranking on P ranks) -------------------------
// mpreid_rr_jaccard above builds the WHOLE index on every rank: the one part of the sharded re-ranking that does not shrink
// as 1/P.  Here rank r builds the columns [c_lo, c_hi) of its column shard only -- the same counting sort (rows cut into the
// same CSC_B blocks, the same packed entries and chunk-boundary table), restricted to a column window -- and the ranks
// exchange (1) the column counts [N] u32, (2) their contiguous piece of the packed index, (3) their rows of the boundary
// table.  Within a column the entries are grouped by row block exactly as in the single build; the order inside a block is
// LDS-atomic arrival order in both, and the Jaccard sum does not depend on it (every row occurs once per column and owns its
// accumulator): outputs are bit-identical (tests/test_gpu_rerank.py::test_sharded_sparse_phases_equal_single_call).
// (n, nq) of the three csc entry points: at least one INDEXED row (nq < n: jaccard_plan divides by the rows per block) and
// packed positions that fit 32 bits
static bool csc_shape_ok(int64_t n, int64_t nq) { return n > 0 && nq >= 0 && nq < n; }
extern "C" int mpreid_rr_csc_chunks(int64_t n, int64_t nq) {
    ARG_CHECK(csc_shape_ok(n, nq));
    return jaccard_plan(n - nq).nchunks;
}

// n * qstride must be below 2^32 for the packed positions (cptr is consumed as u32 positions by the fill and the Jaccard stage)
static int csc_check_packed(const char *who, int64_t n, int qstride) {
    if (csc_packed_ok(n, qstride)) return MPREID_OK;
    mpreid_set_error("%s: n * qstride must be below 2^32 (packed positions)", who);
    return MPREID_ERR_ARG;
}

// step 1: ccnt[c] = number of indexed entries (rows [nq, n)) of every column c in [c_lo, c_hi); chist (mpreid_rr_jaccard_hist_bytes)
// keeps the per-block offsets of those columns for step 2
extern "C" int mpreid_rr_csc_count(int64_t n, int64_t nq, const int32_t *qcnt_all, const int32_t *qidx_all, int qstride,
                                   int64_t c_lo, int64_t c_hi, uint32_t *chist, uint32_t *ccnt, mpreid_stream_t stream_) {
    ARG_CHECK(qcnt_all && qidx_all && chist && ccnt && qstride > 0 && 0 <= c_lo && c_lo <= c_hi && c_hi <= n && csc_shape_ok(n, nq));
    int rc = csc_check_packed("mpreid_rr_csc_count", n, qstride);
    if (rc || c_hi == c_lo) return rc;
    rc = csc_blocked_count(n, nq, qcnt_all, qidx_all, qstride, c_lo, c_hi, chist, ccnt, (hipStream_t)stream_);
    if (rc) return rc;
    LAUNCH_CHECK();
    return MPREID_OK;
}

// step 2 (after the all-gather of the counts): cptr[0 .. n] = exclusive scan of ccnt_all (ccnt_all is zeroed: scratch), then the
// packed entries of the columns [c_lo, c_hi) at their GLOBAL positions cpk[cptr[c_lo] .. cptr[c_hi]) and the rows [c_lo, c_hi)
// of the boundary table hb [n][mpreid_rr_csc_chunks + 1].  chist: as left by step 1.
extern "C" int mpreid_rr_csc_fill(int64_t n, int64_t nq, const int32_t *qcnt_all, const int32_t *qidx_all,
                                  const uint16_t *qval_all, int qstride, int64_t c_lo, int64_t c_hi, uint32_t *ccnt_all,
                                  uint32_t *chist, long long *cptr, uint32_t *cpk, uint32_t *hb, mpreid_stream_t stream_) {
    ARG_CHECK(qcnt_all && qidx_all && qval_all && ccnt_all && chist && cptr && cpk && hb && qstride > 0 && 0 <= c_lo &&
              c_lo <= c_hi && c_hi <= n && csc_shape_ok(n, nq));
    int rc = csc_check_packed("mpreid_rr_csc_fill", n, qstride);
    if (rc) return rc;
    rc = csc_blocked_fill(n, nq, qcnt_all, qidx_all, qval_all, qstride, c_lo, c_hi, ccnt_all, chist, cptr, cpk, hb,
                          (hipStream_t)stream_);
    if (rc) return rc;
    LAUNCH_CHECK();
    return MPREID_OK;
}

// step 3 (after the all-gathers of the index pieces and of the boundary rows): Jaccard + blend of this rank's queries over the
// assembled index -- the second half of mpreid_rr_jaccard
extern "C" int mpreid_rr_jaccard_indexed(int64_t n, int64_t nq, int64_t q_lo, int64_t qrows, const float *d_q, int64_t ld,
                                         const float *rowmax_q, const int32_t *qcnt_all, const int32_t *qidx_all,
                                         const uint16_t *qval_all, int qstride, double lambda_value, const long long *cptr,
                                         const uint32_t *cpk, const uint32_t *hb, float *out, int64_t ldo,
                                         mpreid_stream_t stream_) {
    ARG_CHECK(d_q && rowmax_q && qcnt_all && qidx_all && qval_all && cptr && cpk && hb && out && qrows > 0 && q_lo >= 0 &&
              q_lo + qrows <= nq && ldo >= n - nq);
    return launch_jaccard(n, nq, (int)q_lo, qrows, d_q, ld, rowmax_q, qcnt_all, qidx_all, qval_all, qstride, cptr,
                          (const int *)cpk, nullptr, nullptr, true, lambda_value, out, ldo, nullptr, (hipStream_t)stream_, hb);
}
