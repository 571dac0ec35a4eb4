// pairstats.hip — verification statistics over ALL query x gallery pairs of a resident distance matrix (not in the
// reference): how many positive (same pid) and negative pairs fall between consecutive thresholds.  ROC curves, TPR at a
// false-positive budget and the positive / negative distance histograms are sums and differences of these counts
// (utils/metrics.py: pair_counts, tpr_at_fpr; include/mpreid.h states the definition).
//
// Pure counting: the results are integers, every partial sum is an integer, so the counts do not depend on the launch
// geometry or on the order in which atomics arrive.
//
// Geometry.  Unlike the ranking kernels (one workgroup per row) the matrix is tiled in BOTH directions, so the grid fills
// the chip whatever nq is: a workgroup of 256 threads owns PS_COLS = 1024 consecutive columns and a run of `rows_per` rows
// (the launcher sizes the run for about PS_TARGET_BLOCKS workgroups).  A thread owns four columns of the tile and keeps
// their pids (and camera ids when filtering) in registers while it walks down the rows: label traffic is ng * 8 bytes per
// row BLOCK, not per row.  One row of the tile is one 16-byte load per thread when the matrix allows it (VEC: base pointer
// 16-byte aligned and ld a multiple of 4; a thread's columns are then c0 .. c0 + 3), four coalesced 4-byte loads
// otherwise (columns tid, tid + 256, ...): the same pairs either way.
//
// LDS: bounds [n_bounds] u32 | C privatised copies of the counters [2][n_bounds + 1] u32, C the largest power of two (at
// most 64) that fits PS_COUNTER_WORDS; at the limit of 4096 bounds that is 16 KB + 32 KB with a single copy.  The bucket of
// a key is the number of bounds below it: a branch-free binary search over the LDS bounds with a fixed number of steps,
// run in lockstep for the 16 values (4 rows x 4 columns) a thread has in flight, so that 16 independent LDS reads are
// outstanding per step instead of one dependent chain.  Distances of normalised features fall into a handful of buckets
// in a coarse pass; the privatised copies spread a wave's lanes over up to 64 addresses when the bounds are few.  (A
// wave-aggregated form -- peel off the lanes that hit the first active lane's counter, add the group with one atomic --
// was measured and was slower in every case, also with one copy and 21 non-empty buckets: DESIGN.md section 11.)
// A workgroup holds rows_per * 1024 < 2^32 pairs, so its u32 counters cannot overflow; it flushes the non-zero ones once,
// with 64-bit integer atomicAdds to global memory.
#include "common.h"

constexpr int PS_THREADS = 256;
constexpr int PS_PER_THREAD = 4;
constexpr int PS_COLS = PS_THREADS * PS_PER_THREAD;
constexpr int PS_COUNTER_WORDS = 2 * (MPREID_PAIR_BOUNDS_MAX + 1); // one copy at the limit
constexpr int PS_TARGET_BLOCKS = 2048; // (MPREID_TUNE pair_blocks; 256 ... 2048 measured)
constexpr int PS_ROWS_MAX = 1 << 21; // rows_per * PS_COLS stays below 2^32
constexpr int PS_UNROLL = 4; // rows in flight per thread

// the 32-bit ranking key: the upper half of ev_key (common.h) -- ascending distance, -0 equal to +0
__device__ __forceinline__ unsigned ps_key(float f) { return (unsigned)(ev_key(f, 0u) >> 32); }

template <bool CAM, bool VEC>
__global__ __launch_bounds__(PS_THREADS) void pair_bucket_kernel(const float *__restrict__ dist, int64_t ld, int nq, int ng,
                                                                 const long long *__restrict__ q_pids,
                                                                 const long long *__restrict__ g_pids,
                                                                 const long long *__restrict__ q_cams,
                                                                 const long long *__restrict__ g_cams,
                                                                 const unsigned *__restrict__ bounds, int nb, int step0, int copies,
                                                                 int col_tiles, int rows_per,
                                                                 unsigned long long *__restrict__ counts) {
    extern __shared__ unsigned ps_lds[];
    unsigned *s_bounds = ps_lds;      // [nb]
    unsigned *s_cnt = ps_lds + nb;    // [copies][2][nb + 1]
    const int tid = threadIdx.x, lane = tid & 63;
    const int nbk = nb + 1;
    const int tc = (int)(blockIdx.x % (unsigned)col_tiles), tr = (int)(blockIdx.x / (unsigned)col_tiles);
    const int r0 = tr * rows_per; // (tr < ceil(nq / rows_per): below nq)
    const int r1 = min(nq - r0, rows_per) + r0;
    const int c_tile = tc * PS_COLS;

    for (int t = tid; t < nb; t += PS_THREADS) s_bounds[t] = bounds[t];
    for (int t = tid; t < copies * 2 * nbk; t += PS_THREADS) s_cnt[t] = 0;

    // this thread's columns and their labels
    int col[PS_PER_THREAD];
    bool ok[PS_PER_THREAD];
    long long gp[PS_PER_THREAD], gc[PS_PER_THREAD];
#pragma unroll
    for (int k = 0; k < PS_PER_THREAD; ++k) {
        col[k] = VEC ? c_tile + tid * PS_PER_THREAD + k : c_tile + k * PS_THREADS + tid;
        ok[k] = col[k] < ng;
        gp[k] = ok[k] ? g_pids[col[k]] : 0;
        gc[k] = 0;
        if constexpr (CAM) gc[k] = ok[k] ? g_cams[col[k]] : 0;
    }
    const bool whole = VEC && ok[PS_PER_THREAD - 1]; // all four columns inside: one 16-byte load per row
    __syncthreads();

    unsigned *mine = s_cnt + (lane & (copies - 1)) * 2 * nbk;
    for (int rb = r0; rb < r1; rb += PS_UNROLL) {
        float v[PS_UNROLL][PS_PER_THREAD];
#pragma unroll
        for (int u = 0; u < PS_UNROLL; ++u) {
            const int r = rb + u;
            const float *row = dist + (int64_t)min(r, r1 - 1) * ld; // (rows past the run re-read the last one and are dropped)
            if (whole) {
                const float4 x = *reinterpret_cast<const float4 *>(row + col[0]);
                v[u][0] = x.x; v[u][1] = x.y; v[u][2] = x.z; v[u][3] = x.w;
            } else {
#pragma unroll
                for (int k = 0; k < PS_PER_THREAD; ++k) v[u][k] = ok[k] ? row[col[k]] : 0.0f;
            }
        }
        // lo = number of bounds < key, for all 16 values in lockstep (step0 = the largest power of two <= nb)
        unsigned key[PS_UNROLL][PS_PER_THREAD];
        int lo[PS_UNROLL][PS_PER_THREAD];
#pragma unroll
        for (int u = 0; u < PS_UNROLL; ++u)
#pragma unroll
            for (int k = 0; k < PS_PER_THREAD; ++k) {
                key[u][k] = ps_key(v[u][k]);
                lo[u][k] = 0;
            }
        for (int step = step0; step > 0; step >>= 1) {
#pragma unroll
            for (int u = 0; u < PS_UNROLL; ++u)
#pragma unroll
                for (int k = 0; k < PS_PER_THREAD; ++k) {
                    const int mid = lo[u][k] + step;
                    const bool in = mid <= nb;
                    const unsigned b = s_bounds[in ? mid - 1 : 0];
                    if (in && b < key[u][k]) lo[u][k] = mid;
                }
        }
#pragma unroll
        for (int u = 0; u < PS_UNROLL; ++u) {
            const int r = rb + u;
            if (r >= r1) break; // uniform
            const long long qp = q_pids[r];
            long long qc = 0;
            if constexpr (CAM) qc = q_cams[r];
#pragma unroll
            for (int k = 0; k < PS_PER_THREAD; ++k) {
                const bool pos = gp[k] == qp;
                bool act = ok[k] && isfinite(v[u][k]);
                if constexpr (CAM) act = act && !(pos && gc[k] == qc);
                if (act) atomicAdd(&mine[(pos ? 0 : nbk) + lo[u][k]], 1u);
            }
        }
    }
    __syncthreads();
    // flush: fold the copies, one 64-bit atomic per non-zero counter
    for (int t = tid; t < 2 * nbk; t += PS_THREADS) {
        unsigned s = 0;
        for (int c = 0; c < copies; ++c) s += s_cnt[c * 2 * nbk + t];
        if (s) atomicAdd(&counts[t], (unsigned long long)s);
    }
}

extern "C" int mpreid_pair_bucket_counts(const float *dist_dev, int64_t ld, int nq, int ng, const int64_t *q_pids_dev,
                                         const int64_t *g_pids_dev, const int64_t *q_cams_dev, const int64_t *g_cams_dev,
                                         const uint32_t *bound_keys_dev, int n_bounds, int accumulate,
                                         unsigned long long *counts_dev, mpreid_stream_t stream) {
    ARG_CHECK(n_bounds >= 1 && n_bounds <= MPREID_PAIR_BOUNDS_MAX);
    ARG_CHECK((q_cams_dev == nullptr) == (g_cams_dev == nullptr));
    ARG_CHECK(nq >= 0 && ng >= 0 && ld >= ng);
    ARG_CHECK(bound_keys_dev && counts_dev);
    const int nbk = n_bounds + 1;
    if (!accumulate) HIP_TRY(hipMemsetAsync(counts_dev, 0, (size_t)2 * nbk * sizeof(unsigned long long), (hipStream_t)stream));
    if (nq == 0 || ng == 0) return MPREID_OK;
    ARG_CHECK(dist_dev && q_pids_dev && g_pids_dev);
    const int col_tiles = (ng + PS_COLS - 1) / PS_COLS;
    static const int target = mpreid_tune("pair_blocks", PS_TARGET_BLOCKS);
    int row_blocks = ((target > 0 ? target : 1) + col_tiles - 1) / col_tiles;
    if (row_blocks > nq) row_blocks = nq;
    int rows_per = (nq + row_blocks - 1) / row_blocks;
    if (rows_per > PS_ROWS_MAX) rows_per = PS_ROWS_MAX;
    row_blocks = (nq + rows_per - 1) / rows_per;
    // a workgroup's u32 LDS counters hold at most rows_per * PS_COLS pairs
    if ((uint64_t)rows_per * (uint64_t)PS_COLS >= (1ull << 32)) {
        mpreid_set_error("pair_bucket_counts: a tile of %d rows overflows its counters", rows_per);
        return MPREID_ERR_UNSUPPORTED;
    }
    const int64_t blocks = (int64_t)col_tiles * row_blocks;
    if (blocks > INT32_MAX) {
        mpreid_set_error("pair_bucket_counts: %lld tiles exceed the grid limit", (long long)blocks);
        return MPREID_ERR_UNSUPPORTED;
    }
    int copies = 1;
    while (copies < 64 && 2 * copies * 2 * nbk <= PS_COUNTER_WORDS) copies <<= 1;
    int step0 = 1;
    while (2 * step0 <= n_bounds) step0 <<= 1;
    const size_t lds = ((size_t)n_bounds + (size_t)copies * 2 * nbk) * sizeof(unsigned);
    const bool cam = q_cams_dev != nullptr;
    const bool vec = (reinterpret_cast<uintptr_t>(dist_dev) & 15u) == 0 && (ld & 3) == 0;
    const dim3 grid((unsigned)blocks), block(PS_THREADS);
#define PS_LAUNCH(CAM, VEC)                                                                                               \
    hipLaunchKernelGGL((pair_bucket_kernel<CAM, VEC>), grid, block, lds, (hipStream_t)stream, dist_dev, ld, nq, ng,        \
                       (const long long *)q_pids_dev, (const long long *)g_pids_dev, (const long long *)q_cams_dev,        \
                       (const long long *)g_cams_dev, (const unsigned *)bound_keys_dev, n_bounds, step0, copies,           \
                       col_tiles, rows_per, counts_dev)
    if (cam) {
        if (vec) PS_LAUNCH(true, true); else PS_LAUNCH(true, false);
    } else {
        if (vec) PS_LAUNCH(false, true); else PS_LAUNCH(false, false);
    }
#undef PS_LAUNCH
    LAUNCH_CHECK();
    return MPREID_OK;
}
