// qexpand.hip — query expansion in feature space (AQE on the queries, DBA on the gallery rows): every row becomes the
// similarity-weighted mean of its first k neighbours.  The neighbour lists are mpreid_rank_topk's (idx, dist, cnt) over the
// L2-normalised rows; this file is the aggregation over the RAW rows (steps 4-7 of the definition in include/mpreid.h and
// utils/metrics.py:expand_features), in one launch.
//
// One workgroup per output row.  The row's list becomes (idx, w) in LDS -- thread t < kk turns dist[t] into the weight
// w = max(1 - d / 2, 0) ^ alpha with the rounding sequence of the definition -- and every thread then owns output elements
// (four adjacent ones on the wide path) and walks the list IN LIST ORDER with its own accumulator:
// acc = fadd(acc, fmul(w_j, src[idx_j][e])), separate roundings (__fmul_rn / __fadd_rn: nothing contracts into an FMA), then
// one true divide by float(kk).  Nothing is summed across threads and there are no atomics, so the bits of an element do not
// depend on the workgroup size, on the path or on the grid.
// The kernel is a gather bound by HBM / Infinity Cache (rows * kk * d * 4 bytes in, rows * d * 4 out): the loads of QE_FLY
// list entries are issued before the first of them is used, so a thread keeps QE_FLY rows in flight while the arithmetic
// stays in order.
// Two paths, the same bits: 16-byte loads / stores when src, out and both leading dimensions allow it (the elements past
// d / 4 * 4 go one by one), 4-byte loads otherwise -- no alignment beyond 4 bytes is assumed there.
#include "common.h"

constexpr int QE_FLY = 8; // list entries whose loads are in flight per thread

__device__ __forceinline__ float qe_weight(float dist, int ialpha, float alpha) {
    // the cosine of two unit rows from their squared distance: 0.5 * d is exact, the subtraction rounds once
    const float s = fmaxf(__fsub_rn(1.0f, __fmul_rn(0.5f, dist)), 0.0f);
    if (ialpha == 0) return 1.0f; // alpha == 0: the plain mean, also for s == 0
    if (ialpha > 0) {             // alpha = 1 ... 8: s multiplied alpha - 1 times, left to right
        float w = s;
        for (int i = 1; i < ialpha; ++i) w = __fmul_rn(w, s);
        return w;
    }
    return powf(s, alpha);
}

template <bool VEC>
__global__ __launch_bounds__(256) void qe_aggregate_kernel(const float *__restrict__ src, int d, int64_t ld_src,
                                                           const int *__restrict__ idx, const float *__restrict__ dist,
                                                           const int *__restrict__ cnt, int64_t rows, int k, int ialpha,
                                                           float alpha, float *__restrict__ out, int64_t ld_out) {
    __shared__ int64_t s_off[MPREID_RANK_TOPK_MAX]; // idx_j * ld_src: the 64-bit offset of the neighbour's row
    __shared__ float s_w[MPREID_RANK_TOPK_MAX];
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int64_t r = blockIdx.x; r < rows; r += gridDim.x) {
        int kk = cnt[r];
        kk = kk < 0 ? 0 : (kk > k ? k : kk);
        __syncthreads(); // the previous row's readers are done with the list
        for (int t = tid; t < kk; t += nt) {
            s_off[t] = (int64_t)idx[r * k + t] * ld_src;
            s_w[t] = qe_weight(dist[r * k + t], ialpha, alpha);
        }
        __syncthreads();
        float *orow = out + r * ld_out;
        const float fk = (float)kk;
        const int dv = VEC ? (d >> 2) : 0; // 4-element groups of the wide path
        if constexpr (VEC) {
            for (int c = tid; c < dv; c += nt) {
                float4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
                for (int j0 = 0; j0 < kk; j0 += QE_FLY) {
                    float4 v[QE_FLY];
#pragma unroll
                    for (int u = 0; u < QE_FLY; ++u)
                        if (j0 + u < kk) v[u] = *reinterpret_cast<const float4 *>(src + s_off[j0 + u] + 4 * c);
#pragma unroll
                    for (int u = 0; u < QE_FLY; ++u)
                        if (j0 + u < kk) {
                            const float w = s_w[j0 + u];
                            acc.x = __fadd_rn(acc.x, __fmul_rn(w, v[u].x));
                            acc.y = __fadd_rn(acc.y, __fmul_rn(w, v[u].y));
                            acc.z = __fadd_rn(acc.z, __fmul_rn(w, v[u].z));
                            acc.w = __fadd_rn(acc.w, __fmul_rn(w, v[u].w));
                        }
                }
                float4 o = {0.0f, 0.0f, 0.0f, 0.0f}; // an empty list: zeros
                if (kk > 0) o = {__fdiv_rn(acc.x, fk), __fdiv_rn(acc.y, fk), __fdiv_rn(acc.z, fk), __fdiv_rn(acc.w, fk)};
                *reinterpret_cast<float4 *>(orow + 4 * c) = o;
            }
        }
        for (int e = 4 * dv + tid; e < d; e += nt) {
            float acc = 0.0f;
            for (int j0 = 0; j0 < kk; j0 += QE_FLY) {
                float v[QE_FLY];
#pragma unroll
                for (int u = 0; u < QE_FLY; ++u)
                    if (j0 + u < kk) v[u] = src[s_off[j0 + u] + e];
#pragma unroll
                for (int u = 0; u < QE_FLY; ++u)
                    if (j0 + u < kk) acc = __fadd_rn(acc, __fmul_rn(s_w[j0 + u], v[u]));
            }
            orow[e] = kk > 0 ? __fdiv_rn(acc, fk) : 0.0f;
        }
    }
}

// include/mpreid.h
extern "C" int mpreid_qe_aggregate_f32(const float *src_dev, int64_t n_src, int d, int64_t ld_src, const int32_t *idx_dev,
                                       const float *dist_dev, const int32_t *cnt_dev, int64_t rows, int k, float alpha,
                                       float *out_dev, int64_t ld_out, mpreid_stream_t stream) {
    ARG_CHECK(k >= 1 && d >= 1 && rows >= 0 && n_src >= 0);
    ARG_CHECK(ld_src >= d && ld_out >= d);
    ARG_CHECK(alpha >= 0.0f); // (false for NaN)
    ARG_CHECK(src_dev && idx_dev && dist_dev && cnt_dev && out_dev);
    if (k > MPREID_RANK_TOPK_MAX) {
        mpreid_set_error("mpreid_qe_aggregate_f32: k = %d exceeds MPREID_RANK_TOPK_MAX = %d (the list of a row lives in LDS)", k,
                         MPREID_RANK_TOPK_MAX);
        return MPREID_ERR_UNSUPPORTED;
    }
    if (rows == 0) return MPREID_OK;
    // other rows still read src while a row is written: the two extents must not meet
    if (n_src > 0) {
        const uintptr_t s0 = (uintptr_t)src_dev, s1 = s0 + 4u * (uintptr_t)((n_src - 1) * ld_src + d);
        const uintptr_t o0 = (uintptr_t)out_dev, o1 = o0 + 4u * (uintptr_t)((rows - 1) * ld_out + d);
        if (s0 < o1 && o0 < s1) {
            mpreid_set_error("mpreid_qe_aggregate_f32: out overlaps src (every output row reads other rows of src)");
            return MPREID_ERR_ARG;
        }
    }
    int ialpha = -1; // powf
    if (alpha <= 8.0f && alpha == (float)(int)alpha) ialpha = (int)alpha;
    const bool vec = d >= 4 && ((uintptr_t)src_dev % 16 == 0) && ((uintptr_t)out_dev % 16 == 0) && ld_src % 4 == 0 &&
                     ld_out % 4 == 0;
    const int items = vec ? d / 4 : d; // what a thread owns at a time
    const int threads = items <= 64 ? 64 : (items <= 128 ? 128 : 256);
    const int64_t cap = (int64_t)1 << 20; // workgroups; rows beyond it are taken in further turns of the row loop
    const dim3 grid((unsigned)(rows < cap ? rows : cap)), block((unsigned)threads);
    if (vec)
        hipLaunchKernelGGL((qe_aggregate_kernel<true>), grid, block, 0, (hipStream_t)stream, src_dev, d, ld_src, idx_dev,
                           dist_dev, cnt_dev, rows, k, ialpha, alpha, out_dev, ld_out);
    else
        hipLaunchKernelGGL((qe_aggregate_kernel<false>), grid, block, 0, (hipStream_t)stream, src_dev, d, ld_src, idx_dev,
                           dist_dev, cnt_dev, rows, k, ialpha, alpha, out_dev, ld_out);
    LAUNCH_CHECK();
    return MPREID_OK;
}
