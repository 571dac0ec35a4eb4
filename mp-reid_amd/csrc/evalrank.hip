// evalrank.hip — the ranking part of eval_func (reference utils/metrics.py:28-88) on the GPU.
//
// The reference argsorts every row of distmat (nq x ng) and derives CMC and AP from the positions of the
// gallery items that share the query's pid.  Only those positions are needed, so no sort is done here:
// per query (one 256-thread workgroup)
//   1. collect the relevant items' keys (distance, gallery index) and sort them (bitonic, LDS);
//   2. one pass over the row: every gallery item is dropped into the bucket between two consecutive
//      relevant keys (binary search, LDS histogram);
//   3. prefix sums give, for the t-th relevant item, its 0-based position in the full ascending
//      (value, index) order — exactly the position a stable argsort gives it.
// HBM-bound: 4*nq*ng bytes read once (+ pids); Market-1501 scale: 214 MB.
// The host finishes CMC / AP from the positions (float64, numpy's pairwise order) — utils/metrics.py.
// eval_rank_kernel<true, *> does the same under the Market-1501 protocol (same-identity same-camera gallery items removed).
// eval_rank_kernel<*, true> ranks a batch of (split, query) pairs over ONE resident matrix in one launch: a pair's row is
// a row of the matrix read through the split's list of columns (multi-trial protocols: VehicleID, RegDB).
#include "common.h"
#include <vector>

constexpr int EV_CAP_MAX = 8192; // max relevant gallery items per query handled on the GPU (64 KB of keys + 32 KB of counters)
constexpr int EV_HIST_MIN = 2112; // counter words of the smallest instance: room for privatised copies of a short bucket list

// pos_out [nq][rcap] int32 ascending positions (padded with -1), cnt_out [nq] (= -1 when the query has more
// than min(rcap, cap) relevant items: the caller falls back to the host for that row)
// Dynamic LDS: rel [cap] u64 | hist [hw] u32, cap a power of two >= 64, hw = max(cap + 1, EV_HIST_MIN).
// Step 2's counters are PRIVATISED: with R relevant items there are R + 1 buckets and C = the largest power of two with
// C * (R + 1) <= hw (at most 64) copies of them, copy = lane & (C - 1).  Round 5's single copy took one LDS atomic per
// gallery item into ~22 addresses (Market-1501: ~21 relevant items per query): up to 64 lanes of an instruction on one
// address, serialised by the LDS atomic unit; with R < 32 every lane owns its copy and no two lanes ever collide.
//
// CAM = true is the Market-1501 protocol (the filter the reference promises at utils/metrics.py:29-31, keeps commented out
// at :54 and runs at processor/processor_uniprompt_stage2.py:476-505): gallery items with the query's pid AND the query's
// camera are JUNK -- removed from the ranking.  Junk items are pid hits, so step 1 reads g_cams only for the hits and the
// sorted list holds relevant and junk keys together (R = pid hits).  The junk flag is bit 0 of the key's index field,
// BELOW the gallery index (idx = 2 j + junk, j < 2^31): j is unique, so two keys never compare on the flag and the list
// keeps its (distance, gallery index) order on ties; no second LDS array follows the sort's swaps.  Step 2 buckets every
// gallery item as before (junk and relevant items land in their own buckets); step 3 subtracts from a relevant item's
// position the number of junk keys sorted in front of it and writes the relevant entries compacted.
// CAM = false is the kernel without the filter: q_cams / g_cams are not read (the launcher passes null) and its
// instructions are those the non-template kernel compiled to.
//
// SPLITS = true: block b is the PAIR b of a batch -- query row q_row[b] of the resident matrix against the gallery list
// g_idx[g_off[s] .. g_off[s + 1]) of split s = q_split[b].  q_pids / q_cams / pos_out / cnt_out are indexed by the pair;
// g_pids / g_cams are the labels of the list entries (pre-gathered by the caller, aligned with g_idx), so step 1 reads them
// coalesced and only the distances go through the index list: item j of the row is dist[q_row[b]][g_idx[g_off[s] + j]].
// The key's index field is j, the POSITION IN THE LIST (not the matrix column): the positions are those of a stable
// argsort of the gathered row, whatever order the list is in.  `ng` is unused (every split has its own length).
// SPLITS = false reads none of the four trailing arguments (the launchers pass null): the existing instantiations keep
// their instructions.
template <bool CAM, bool SPLITS>
__global__ __launch_bounds__(256) void eval_rank_kernel(const float *__restrict__ dist, int64_t ld, int nq, int ng,
                                                        const long long *__restrict__ q_pids,
                                                        const long long *__restrict__ g_pids,
                                                        const long long *__restrict__ q_cams,
                                                        const long long *__restrict__ g_cams, int rcap, int cap, int hw,
                                                        int *__restrict__ pos_out, int *__restrict__ cnt_out,
                                                        const int *__restrict__ q_row, const int *__restrict__ q_split,
                                                        const long long *__restrict__ g_off,
                                                        const int *__restrict__ g_idx) {
    extern __shared__ unsigned long long ev_lds[];
    unsigned long long *rel = ev_lds;
    unsigned *hist = reinterpret_cast<unsigned *>(ev_lds + cap);
    __shared__ unsigned s_cnt;
    __shared__ int s_wave[CAM ? 8 : 4]; // [4..7]: wave totals of the junk flags
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = blockIdx.x;
    const float *row = dist + (int64_t)(SPLITS ? q_row[q] : q) * ld;
    if constexpr (SPLITS) { // this pair's split: its slice of the gallery lists and its length
        const int s = q_split[q];
        const long long o0 = g_off[s];
        ng = (int)(g_off[s + 1] - o0);
        g_pids += o0;
        g_idx += o0;
        if constexpr (CAM) g_cams += o0;
    }
    const long long pid = q_pids[q];
    long long cam = 0;
    if constexpr (CAM) cam = q_cams[q];
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    // 1. relevant items (wave-aggregated reservation: one LDS atomic per wave and 64 items)
    for (int j0 = 0; j0 < ng; j0 += 256) {
        const int j = j0 + tid;
        const bool hit = j < ng && g_pids[j] == pid;
        const unsigned long long m = __ballot(hit);
        if (m) {
            unsigned base = 0;
            if (lane == 0) base = atomicAdd(&s_cnt, (unsigned)__popcll(m));
            base = __shfl(base, 0, 64);
            if (hit) {
                const unsigned p = base + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
                if constexpr (CAM) {
                    if (p < (unsigned)cap)
                        rel[p] = ev_key(row[SPLITS ? g_idx[j] : j], ((unsigned)j << 1) | (g_cams[j] == cam ? 1u : 0u));
                } else {
                    if (p < (unsigned)cap) rel[p] = ev_key(row[SPLITS ? g_idx[j] : j], (unsigned)j);
                }
            }
        }
    }
    __syncthreads();
    const int R = (int)s_cnt;
    if (R > cap || R > rcap) {
        if (tid == 0) cnt_out[q] = -1;
        return;
    }
    if constexpr (!CAM)
        if (tid == 0) cnt_out[q] = R;
    if (R == 0) {
        if constexpr (CAM)
            if (tid == 0) cnt_out[q] = 0;
        for (int t = tid; t < rcap; t += 256) pos_out[(int64_t)q * rcap + t] = -1;
        return;
    }
    int npow = 1;
    while (npow < R) npow <<= 1;
    for (int t = R + tid; t < npow; t += 256) rel[t] = ~0ull; // padding sorts last
    const int nb = R + 1;
    int C = 1;
    while (C < 64 && 2 * C * nb <= hw) C <<= 1;
    for (int t = tid; t < C * nb; t += 256) hist[t] = 0;
    __syncthreads();
    for (int size = 2; size <= npow; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < npow; t += 256) {
                const int partner = t ^ stride;
                if (partner > t) {
                    const unsigned long long a = rel[t], b = rel[partner];
                    const bool up = ((t & size) == 0);
                    if ((a > b) == up) {
                        rel[t] = b;
                        rel[partner] = a;
                    }
                }
            }
            __syncthreads();
        }
    // 2. bucket every gallery item: b = number of relevant keys < key_j (a relevant item t lands in bucket t)
    unsigned *mine = hist + (lane & (C - 1)) * nb;
    for (int j = tid; j < ng; j += 256) {
        // (CAM: flag bit clear -- the item's own list entry, flagged or not, is still the first one >= k)
        const unsigned long long k = ev_key(row[SPLITS ? g_idx[j] : j], CAM ? (unsigned)j << 1 : (unsigned)j);
        int lo = 0, hi = R; // first t with rel[t] >= k
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (rel[mid] < k) lo = mid + 1; else hi = mid;
        }
        atomicAdd(&mine[lo], 1u); // items with key in (rel[lo-1], rel[lo]]
    }
    __syncthreads();
    if (C > 1) { // fold the copies into copy 0 (thread t touches column t of every copy and nothing else)
        for (int t = tid; t < nb; t += 256) {
            unsigned s = 0;
            for (int c = 0; c < C; ++c) s += hist[c * nb + t];
            hist[t] = s;
        }
        __syncthreads();
    }
    // 3. position of relevant item t = number of items with a smaller key = sum_{b<=t} hist[b] - 1 (itself)
    //    (CAM: minus the junk keys among rel[0..t), written at index t - that number; junk entries are not written)
    unsigned run = 0;
    int jrun = 0;
    for (int t0 = 0; t0 < R; t0 += 256) {
        const int t = t0 + tid;
        const int v = (t < R) ? (int)hist[t] : 0;
        int jf = 0;
        if constexpr (CAM) jf = (t < R) ? (int)(rel[t] & 1ull) : 0;
        // block inclusive scan
        int x = v, jx = jf;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int y = __shfl_up(x, off, 64);
            if (lane >= off) x += y;
            if constexpr (CAM) {
                const int jy = __shfl_up(jx, off, 64);
                if (lane >= off) jx += jy;
            }
        }
        __syncthreads();
        if (lane == 63) {
            s_wave[wave] = x;
            if constexpr (CAM) s_wave[4 + wave] = jx;
        }
        __syncthreads();
        int base = 0, tot = 0, jbase = 0, jtot = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            if (w < wave) base += s_wave[w];
            tot += s_wave[w];
            if constexpr (CAM) {
                if (w < wave) jbase += s_wave[4 + w];
                jtot += s_wave[4 + w];
            }
        }
        if constexpr (CAM) {
            const int jb = jrun + jbase + jx; // junk keys among rel[0..t]
            if (t < R && !jf) pos_out[(int64_t)q * rcap + (t - jb)] = (int)(run + (unsigned)(base + x)) - 1 - jb;
            jrun += jtot;
        } else {
            if (t < R) pos_out[(int64_t)q * rcap + t] = (int)(run + (unsigned)(base + x)) - 1;
        }
        run += (unsigned)tot;
        __syncthreads();
    }
    const int nrel = R - jrun;
    if constexpr (CAM)
        if (tid == 0) cnt_out[q] = nrel;
    for (int t = nrel + tid; t < rcap; t += 256) pos_out[(int64_t)q * rcap + t] = -1;
}

// the launch geometry of every instantiation: cap (LDS entries of the sorted list), hw (counter words), LDS bytes
static inline size_t ev_geometry(int rcap, int *cap_out, int *hw_out) {
    int cap = 64;
    while (cap < rcap && cap < EV_CAP_MAX) cap <<= 1;
    const int hw = cap + 1 > EV_HIST_MIN ? cap + 1 : EV_HIST_MIN;
    *cap_out = cap;
    *hw_out = hw;
    return (size_t)cap * 8 + (size_t)hw * 4;
}

// The one launch of every instantiation: geometry, dynamic LDS, profiler bracket (filed under (nq, prof_n, prof_k) with
// `work` algorithmic bytes), launch.  ng: the gallery size, 0 with SPLITS (the lists g_off / g_idx give it per pair).
template <bool CAM, bool SPLITS>
static int launch_eval_rank(const float *dist, int64_t ld, int nq, int ng, const int64_t *q_pids, const int64_t *g_pids,
                            const int64_t *q_camids, const int64_t *g_camids, int rcap, int32_t *pos_out, int32_t *cnt_out,
                            const int32_t *q_row, const int32_t *q_split, const int64_t *g_off, const int32_t *g_idx,
                            int prof_n, int prof_k, double work, hipStream_t stream) {
    int cap, hw;
    const size_t lds = ev_geometry(rcap, &cap, &hw);
    const int rc = mpreid_dyn_lds(eval_rank_kernel<CAM, SPLITS>, lds);
    if (rc != MPREID_OK) return rc;
    void *ptok = mpreid_prof_begin(stream);
    hipLaunchKernelGGL((eval_rank_kernel<CAM, SPLITS>), dim3((unsigned)nq), dim3(256), lds, stream, dist, ld, nq, ng,
                       (const long long *)q_pids, (const long long *)g_pids, (const long long *)q_camids,
                       (const long long *)g_camids, rcap, cap, hw, pos_out, cnt_out, (const int *)q_row, (const int *)q_split,
                       (const long long *)g_off, (const int *)g_idx);
    mpreid_prof_end(ptok, stream, MPREID_PROF_EVALRANK, nq, prof_n, prof_k, work);
    LAUNCH_CHECK();
    return MPREID_OK;
}

extern "C" int mpreid_eval_rank_positions(const float *dist_dev, int64_t ld, int nq, int ng, const int64_t *q_pids_dev,
                                          const int64_t *g_pids_dev, int rcap, int32_t *pos_out_dev,
                                          int32_t *cnt_out_dev, mpreid_stream_t stream) {
    ARG_CHECK(dist_dev && q_pids_dev && g_pids_dev && pos_out_dev && cnt_out_dev && nq > 0 && ng > 0 && ld >= ng &&
              rcap > 0);
    return launch_eval_rank<false, false>(dist_dev, ld, nq, ng, q_pids_dev, g_pids_dev, nullptr, nullptr, rcap, pos_out_dev,
                                          cnt_out_dev, nullptr, nullptr, nullptr, nullptr, ng, 0,
                                          4.0 * (double)nq * (double)ng, (hipStream_t)stream);
}

extern "C" int mpreid_eval_rank_positions_cam(const float *dist_dev, int64_t ld, int nq, int ng,
                                              const int64_t *q_pids_dev, const int64_t *g_pids_dev,
                                              const int64_t *q_camids_dev, const int64_t *g_camids_dev, int rcap,
                                              int32_t *pos_out_dev, int32_t *cnt_out_dev, mpreid_stream_t stream) {
    ARG_CHECK(dist_dev && q_pids_dev && g_pids_dev && q_camids_dev && g_camids_dev && pos_out_dev && cnt_out_dev &&
              nq > 0 && ng > 0 && ld >= ng && rcap > 0);
    return launch_eval_rank<true, false>(dist_dev, ld, nq, ng, q_pids_dev, g_pids_dev, q_camids_dev, g_camids_dev, rcap,
                                         pos_out_dev, cnt_out_dev, nullptr, nullptr, nullptr, nullptr, ng, 0,
                                         4.0 * (double)nq * (double)ng, (hipStream_t)stream);
}

// A batch of (split, query) pairs over one resident matrix: include/mpreid.h.  One launch, one block per pair.
extern "C" int mpreid_eval_rank_positions_splits(const float *dist_dev, int64_t ld, int64_t n_rows, int64_t n_cols, int nqt,
                                                 const int32_t *q_row_dev, const int32_t *q_split_dev,
                                                 const int64_t *q_pids_dev, const int64_t *q_camids_dev, int n_splits,
                                                 const int64_t *g_off_dev, const int32_t *g_idx_dev,
                                                 const int64_t *g_pids_dev, const int64_t *g_camids_dev, int rcap,
                                                 int32_t *pos_out_dev, int32_t *cnt_out_dev, mpreid_stream_t stream) {
    ARG_CHECK(dist_dev && q_row_dev && q_split_dev && q_pids_dev && g_off_dev && g_idx_dev && g_pids_dev && pos_out_dev &&
              cnt_out_dev);
    ARG_CHECK((q_camids_dev == nullptr) == (g_camids_dev == nullptr));
    ARG_CHECK(n_rows > 0 && n_rows <= INT32_MAX && n_cols > 0 && n_cols <= INT32_MAX && ld >= n_cols && nqt > 0 &&
              n_splits > 0 && rcap > 0);
    // profiling runs only: the work figure (4 bytes per gathered distance, summed over the pairs) needs the split of
    // every pair and the list lengths, which live on the device -- two small blocking copies BEFORE the timed interval
    double work = 0.0;
    if (mpreid_prof_active()) {
        std::vector<int32_t> qs((size_t)nqt);
        std::vector<int64_t> off((size_t)n_splits + 1);
        HIP_TRY(hipMemcpyAsync(qs.data(), q_split_dev, qs.size() * 4, hipMemcpyDeviceToHost, (hipStream_t)stream));
        HIP_TRY(hipMemcpyAsync(off.data(), g_off_dev, off.size() * 8, hipMemcpyDeviceToHost, (hipStream_t)stream));
        HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
        for (int b = 0; b < nqt; ++b)
            if (qs[b] >= 0 && qs[b] < n_splits) work += 4.0 * (double)(off[qs[b] + 1] - off[qs[b]]);
    }
    const auto launch = q_camids_dev ? launch_eval_rank<true, true> : launch_eval_rank<false, true>;
    return launch(dist_dev, ld, nqt, 0, q_pids_dev, g_pids_dev, q_camids_dev, g_camids_dev, rcap, pos_out_dev, cnt_out_dev,
                  q_row_dev, q_split_dev, g_off_dev, g_idx_dev, (int)n_cols, n_splits, work, (hipStream_t)stream);
}
