// ranklist.hip — ranked gallery lists: the first k entries of every row of a distance matrix in ascending
// (distance, gallery index) order -- np.argsort(distmat, axis=1)[:, :k] of reference utils/metrics.py:39, made stable.
//
// One 256-thread workgroup per query row (as eval_rank_kernel).  An item's key is ev_key(dist, 2 * gidx + z) with gidx its
// GLOBAL gallery index (col0 + j) and z = 1 iff the entry's bits are those of -0.0: gidx is unique, so two keys never
// compare on z and the order is the (distance, gallery index) order of the definition; every key of a row is distinct,
// and the entry's own bits come back out of the key (no second array follows the sort).
//
// Selection = MSB radix select over the 64-bit keys, digits of 12 | 12 | 8 bits over the distance half and 12 | 12 | 8 over
// the index half (LDS histogram of 4096 counters):
//   pass p: count, per digit value, the items whose key agrees with the prefix found so far; the digit whose bucket holds
//           the kk-th key (kk = min(k, kept items)) extends the prefix; `below` = keys smaller than the whole prefix.
//   stop as soon as below + |bucket| <= RL_SEL (2048): all keys <= (prefix, all ones) are then gathered into LDS, sorted
//           (bitonic, distinct keys) and the first kk are written.
// Keys are distinct, so the bucket of the last pass holds ONE key and the loop always ends: any number of entries equal to
// the k-th distance is handled by the index digits, not by a candidate array (a row of equal distances: 5 passes).  Random
// distances in a narrow range (normalised features) stop after the second pass: 3 reads of the row, gather included.
// The counters are LDS atomics (sums: order-free); the gather order is arbitrary and is erased by the sort.
// carry: the list already in idx / val (cnt entries, built from OTHER columns) joins the row's items as ready keys in LDS.
// CAM: gallery items with the query's pid AND the query's camera (mpreid_eval_rank_positions_cam's junk) are skipped in
// every pass; the labels [ng] are shared by all rows and stay in L2.
// Loads are 4-byte scalar-per-lane loads: no alignment is assumed of ld, the row pointer or ng.
#include "common.h"

constexpr int RL_BINS = 4096; // counters of one radix pass (12-bit digit)
constexpr int RL_SEL = 2048;  // keys gathered and sorted in LDS (>= MPREID_RANK_TOPK_MAX)
static_assert(RL_SEL >= MPREID_RANK_TOPK_MAX && RL_BINS % 256 == 0, "geometry");

__device__ __forceinline__ unsigned long long rl_key(float f, unsigned gidx) {
    return ev_key(f, (gidx << 1) | (__float_as_uint(f) == 0x80000000u ? 1u : 0u));
}

// every kept item of the row, then the carried keys: f(key)
template <bool CAM, typename F>
__device__ __forceinline__ void rl_scan(const float *row, unsigned ng, unsigned col0, const long long *g_pids,
                                        const long long *g_cams, long long pid, long long cam,
                                        const unsigned long long *car, int cc, int tid, F f) {
    for (unsigned j = (unsigned)tid; j < ng; j += 256u) {
        if constexpr (CAM) {
            if (g_pids[j] == pid && g_cams[j] == cam) continue; // junk
        }
        f(rl_key(row[j], col0 + j));
    }
    for (int t = tid; t < cc; t += 256) f(car[t]);
}

template <bool CAM>
__global__ __launch_bounds__(256) void rank_topk_kernel(const float *__restrict__ dist, int64_t ld, int ng, unsigned col0,
                                                        int k, const long long *__restrict__ q_pids,
                                                        const long long *__restrict__ g_pids,
                                                        const long long *__restrict__ q_cams,
                                                        const long long *__restrict__ g_cams, int carry, int *idx_io,
                                                        float *val_io, int *cnt_io) {
    __shared__ unsigned long long sel[RL_SEL];
    __shared__ unsigned long long car[MPREID_RANK_TOPK_MAX];
    __shared__ unsigned hist[RL_BINS];
    __shared__ unsigned s_wave[4];
    __shared__ unsigned s_bin, s_before, s_h, s_n;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = blockIdx.x;
    const float *row = dist + (int64_t)q * ld;
    int *idx_row = idx_io + (int64_t)q * k;
    float *val_row = val_io + (int64_t)q * k;
    long long pid = 0, cam = 0;
    if constexpr (CAM) {
        pid = q_pids[q];
        cam = q_cams[q];
    }
    int cc = 0; // carried entries: taken by count
    if (carry) {
        cc = cnt_io[q];
        cc = cc < 0 ? 0 : (cc > k ? k : cc);
        for (int t = tid; t < cc; t += 256) car[t] = rl_key(val_row[t], (unsigned)idx_row[t]);
    }
    unsigned long long prefix = 0; // the key's bits above `shift` + `bits`, once a pass has run
    unsigned below = 0;            // keys smaller than every key with that prefix
    unsigned kk = 0;
    int shift = 64;
    for (int p = 0; p < 6; ++p) {
        const int bits = (p % 3 == 2) ? 8 : 12;
        shift -= bits;
        for (int t = tid; t < RL_BINS; t += 256) hist[t] = 0;
        __syncthreads(); // (also orders the carried keys' stores and the previous pass's reads of s_bin / s_before / s_h)
        const unsigned mask = (1u << bits) - 1u;
        if (p == 0) {
            rl_scan<CAM>(row, (unsigned)ng, col0, g_pids, g_cams, pid, cam, car, cc, tid,
                         [&](unsigned long long key) { atomicAdd(&hist[(unsigned)(key >> shift) & mask], 1u); });
        } else {
            const int up = shift + bits;
            rl_scan<CAM>(row, (unsigned)ng, col0, g_pids, g_cams, pid, cam, car, cc, tid, [&](unsigned long long key) {
                if ((key >> up) == prefix) atomicAdd(&hist[(unsigned)(key >> shift) & mask], 1u);
            });
        }
        __syncthreads();
        // thread t owns the counters [16 t, 16 t + 16): block exclusive scan of their sums
        constexpr int PER = RL_BINS / 256;
        unsigned s = 0;
        for (int i = 0; i < PER; ++i) s += hist[tid * PER + i];
        unsigned x = s;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned y = __shfl_up(x, off, 64);
            if (lane >= off) x += y;
        }
        if (lane == 63) s_wave[wave] = x;
        __syncthreads();
        unsigned base = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            if (w < wave) base += s_wave[w];
            tot += s_wave[w];
        }
        if (p == 0) {
            kk = tot < (unsigned)k ? tot : (unsigned)k;
            if (kk == 0) break; // nothing kept and nothing carried (uniform)
        }
        // the bucket of the kk-th key: below + (counters before it) < kk <= below + (counters through it); one thread finds it
        unsigned run = below + base + (x - s);
        if (run < kk && kk <= run + s) {
            for (int i = 0; i < PER; ++i) {
                const unsigned h = hist[tid * PER + i];
                if (kk <= run + h) {
                    s_bin = (unsigned)(tid * PER + i);
                    s_before = run;
                    s_h = h;
                    break;
                }
                run += h;
            }
        }
        __syncthreads();
        below = s_before;
        prefix = (prefix << bits) | s_bin;
        if (below + s_h <= (unsigned)RL_SEL) break; // (the last pass: s_h = 1, below + 1 = kk <= 1024)
    }
    if (kk > 0) {
        // gather every key <= (prefix, all ones): below + s_h of them, at most RL_SEL
        if (tid == 0) s_n = 0;
        __syncthreads();
        rl_scan<CAM>(row, (unsigned)ng, col0, g_pids, g_cams, pid, cam, car, cc, tid, [&](unsigned long long key) {
            if ((key >> shift) <= prefix) {
                const unsigned slot = atomicAdd(&s_n, 1u);
                if (slot < (unsigned)RL_SEL) sel[slot] = key;
            }
        });
        __syncthreads();
        const int n = (int)(s_n < (unsigned)RL_SEL ? s_n : (unsigned)RL_SEL);
        int npow = 1;
        while (npow < n) npow <<= 1;
        for (int t = n + tid; t < npow; t += 256) sel[t] = ~0ull; // padding sorts last
        __syncthreads();
        for (int size = 2; size <= npow; size <<= 1)
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                for (int t = tid; t < npow; t += 256) {
                    const int partner = t ^ stride;
                    if (partner > t) {
                        const unsigned long long a = sel[t], b = sel[partner];
                        const bool up = ((t & size) == 0);
                        if ((a > b) == up) {
                            sel[t] = b;
                            sel[partner] = a;
                        }
                    }
                }
                __syncthreads();
            }
        for (int t = tid; t < (int)kk; t += 256) {
            const unsigned long long key = sel[t];
            const unsigned lo = (unsigned)key, u = (unsigned)(key >> 32);
            idx_row[t] = (int)(lo >> 1);
            // the entry's own bits: -0 by the flag, everything else by inverting ev_key's map
            val_row[t] = __uint_as_float((lo & 1u) ? 0x80000000u : ((u & 0x80000000u) ? (u ^ 0x80000000u) : ~u));
        }
    }
    for (int t = (int)kk + tid; t < k; t += 256) {
        idx_row[t] = -1;
        val_row[t] = __uint_as_float(0x7f800000u); // +inf
    }
    if (tid == 0) cnt_io[q] = (int)kk;
}

// include/mpreid.h
extern "C" int mpreid_rank_topk(const float *dist_dev, int64_t ld, int nq, int ng, int64_t col0, int k,
                                const int64_t *q_pids_dev, const int64_t *g_pids_dev, const int64_t *q_camids_dev,
                                const int64_t *g_camids_dev, int carry, int32_t *idx_io_dev, float *val_io_dev,
                                int32_t *cnt_io_dev, mpreid_stream_t stream) {
    ARG_CHECK(k >= 1 && nq >= 0 && ng >= 0);
    if (k > MPREID_RANK_TOPK_MAX) {
        mpreid_set_error("mpreid_rank_topk: k = %d exceeds MPREID_RANK_TOPK_MAX = %d (the sorted list of a row lives in LDS)",
                         k, MPREID_RANK_TOPK_MAX);
        return MPREID_ERR_UNSUPPORTED;
    }
    const int n_lab = (q_pids_dev != nullptr) + (g_pids_dev != nullptr) + (q_camids_dev != nullptr) + (g_camids_dev != nullptr);
    ARG_CHECK(n_lab == 0 || n_lab == 4);
    ARG_CHECK(col0 >= 0 && col0 + (int64_t)ng < ((int64_t)1 << 31));
    ARG_CHECK(idx_io_dev && val_io_dev && cnt_io_dev);
    ARG_CHECK(ng == 0 || (dist_dev && ld >= ng));
    if (nq == 0 || (ng == 0 && carry)) return MPREID_OK;
    const dim3 grid((unsigned)nq), block(256);
    if (n_lab == 4)
        hipLaunchKernelGGL((rank_topk_kernel<true>), grid, block, 0, (hipStream_t)stream, dist_dev, ld, ng, (unsigned)col0,
                           k, (const long long *)q_pids_dev, (const long long *)g_pids_dev,
                           (const long long *)q_camids_dev, (const long long *)g_camids_dev, carry ? 1 : 0, idx_io_dev,
                           val_io_dev, cnt_io_dev);
    else
        hipLaunchKernelGGL((rank_topk_kernel<false>), grid, block, 0, (hipStream_t)stream, dist_dev, ld, ng,
                           (unsigned)col0, k, (const long long *)nullptr, (const long long *)nullptr,
                           (const long long *)nullptr, (const long long *)nullptr, carry ? 1 : 0, idx_io_dev, val_io_dev,
                           cnt_io_dev);
    LAUNCH_CHECK();
    return MPREID_OK;
}
