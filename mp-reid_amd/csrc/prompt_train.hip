// prompt_train.hip — stage-1 prompt learning around the text tower (include/mpreid.h): the symmetric supervised contrastive
// loss with its gradients, the context gradient as a segment sum of the prompt gradient, and the Adam / AdamW step.  fp32
// throughout, no atomics, every sum in a fixed order: the same bits from run to run.  The kernels are small and latency-bound
// (batch 64: a 64 x 64 logit matrix); what counts is the number of launches, four for the loss and one for each of the others.
#include "common.h"

#include <cmath>

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// S = img . txt^T and its transpose: a 16 x 16 tile of S per workgroup, one entry per thread, one fmaf chain over the features
// ---------------------------------------------------------------------------------------------------------------------
constexpr int SC_T = 16, SC_K = 32;

__global__ __launch_bounds__(SC_T * SC_T) void supcon_logits_kernel(const float *__restrict__ img, const float *__restrict__ txt,
                                                                    int B, int D, float *__restrict__ S, float *__restrict__ St) {
    __shared__ float As[SC_T][SC_K + 1], Bs[SC_T][SC_K + 1];
    const int tx = threadIdx.x & (SC_T - 1), ty = threadIdx.x / SC_T;
    const int a0 = blockIdx.y * SC_T, b0 = blockIdx.x * SC_T;
    float acc = 0.f;
    for (int k0 = 0; k0 < D; k0 += SC_K) {
        for (int i = threadIdx.x; i < SC_T * SC_K; i += SC_T * SC_T) {
            const int r = i / SC_K, c = i - r * SC_K;
            const bool kin = k0 + c < D;
            As[r][c] = (kin && a0 + r < B) ? img[(int64_t)(a0 + r) * D + k0 + c] : 0.f;
            Bs[r][c] = (kin && b0 + r < B) ? txt[(int64_t)(b0 + r) * D + k0 + c] : 0.f;
        }
        __syncthreads();
        const int kn = min(SC_K, D - k0);   // (the zero padding is never added: a chain of exactly D terms)
        for (int c = 0; c < kn; ++c) acc = fmaf(As[ty][c], Bs[tx][c], acc);
        __syncthreads();
    }
    const int a = a0 + ty, b = b0 + tx;
    if (a < B && b < B) {
        S[(int64_t)a * B + b] = acc;
        St[(int64_t)b * B + a] = acc;
    }
}

// Row statistics, one wave per row r of the [2B][B] matrix S | S^T (row B + b is column b of S): the maximum, the log of the
// sum of exp(entry - maximum), 1 / n and the row's term of its loss, (1 / n) sum over the same-label entries of log-softmax.
__global__ __launch_bounds__(256) void supcon_stats_kernel(const float *__restrict__ S2, const int64_t *__restrict__ labels, int B,
                                                           float *__restrict__ rmax, float *__restrict__ rlog,
                                                           float *__restrict__ rinv, float *__restrict__ term) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= 2 * B) return;
    const float *row = S2 + (int64_t)r * B;
    const int64_t mine = labels[r < B ? r : r - B];
    float m = -INFINITY;
    for (int j = lane; j < B; j += 64) m = fmaxf(m, row[j]);
    m = wave_bfly_max(m);
    float s = 0.f;
    for (int j = lane; j < B; j += 64) s += expf(row[j] - m);
    const float lg = logf(wave_bfly_add(s));
    float pos = 0.f, cnt = 0.f;
    for (int j = lane; j < B; j += 64)
        if (labels[j] == mine) {
            pos += (row[j] - m) - lg;
            cnt += 1.f;
        }
    pos = wave_bfly_add(pos);
    cnt = wave_bfly_add(cnt);   // >= 1: the row's own entry (exact: at most 1024)
    if (lane == 0) {
        rmax[r] = m;
        rlog[r] = lg;
        rinv[r] = __fdiv_rn(1.0f, cnt);
        term[r] = __fdiv_rn(pos, cnt);
    }
}

// loss[d] = -(sum over the B row terms of direction d) / B, one workgroup
__global__ __launch_bounds__(256) void supcon_loss_kernel(const float *__restrict__ term, int B, float *__restrict__ loss) {
    __shared__ float red[2][4];
    const int tid = threadIdx.x;
    float s[2] = {0.f, 0.f};
    for (int d = 0; d < 2; ++d) {
        for (int j = tid; j < B; j += 256) s[d] += term[d * B + j];
        s[d] = wave_bfly_add(s[d]);
        if ((tid & 63) == 0) red[d][tid >> 6] = s[d];
    }
    __syncthreads();
    if (tid < 2) loss[tid] = -__fdiv_rn(((red[tid][0] + red[tid][1]) + red[tid][2]) + red[tid][3], (float)B);
}

// One gradient row per workgroup.  side 0: d_img[a] = sum_b G_ab txt[b]; side 1: d_txt[b] = sum_a G_ab img[a].  The row of G
// (of G^T) goes to LDS first, computed from the row of S (of S^T) and both sides' statistics, the same expression either way.
// dirs: bit 0 = the row-softmax term of G (loss_i2t), bit 1 = the column-softmax term (loss_t2i).
__global__ __launch_bounds__(256) void supcon_grad_kernel(const float *__restrict__ S2, const int64_t *__restrict__ labels,
                                                          const float *__restrict__ rmax, const float *__restrict__ rlog,
                                                          const float *__restrict__ rinv, const float *__restrict__ img,
                                                          const float *__restrict__ txt, int B, int D, int side0, int dirs,
                                                          float *__restrict__ d_img, float *__restrict__ d_txt) {
    __shared__ float Gs[MPREID_SUPCON_MAX_BATCH];
    const int tid = threadIdx.x, r = blockIdx.x, side = side0 + blockIdx.y;
    const float *row = S2 + ((int64_t)side * B + r) * B;
    const int64_t mine = labels[r];
    const int own = side * B + r;          // this row's statistics: softmax over ITS entries
    const int other0 = (1 - side) * B;     // entry j's statistics in the other direction
    const float inv_b = __fdiv_rn(1.0f, (float)B);
    for (int j = tid; j < B; j += 256) {
        const float s = row[j];
        const float mk = labels[j] == mine ? 1.f : 0.f;
        const float t_own = mk * rinv[own] - expf((s - rmax[own]) - rlog[own]);
        const float t_oth = mk * rinv[other0 + j] - expf((s - rmax[other0 + j]) - rlog[other0 + j]);
        const float t_p = side == 0 ? t_own : t_oth, t_q = side == 0 ? t_oth : t_own;
        Gs[j] = -inv_b * (dirs == 3 ? t_p + t_q : (dirs == 1 ? t_p : t_q));   // (one order on both sides: G_ab has one value)
    }
    __syncthreads();
    const float *X = side == 0 ? txt : img;
    float *out = (side == 0 ? d_img : d_txt) + (int64_t)r * D;
    for (int e = tid; e < D; e += 256) {
        float acc = 0.f;
        for (int j = 0; j < B; ++j) acc = fmaf(Gs[j], X[(int64_t)j * D + e], acc);
        out[e] = acc;
    }
}

struct SupconLayout {
    size_t s2, rmax, rlog, rinv, term, total;
};

SupconLayout supcon_layout(int B) {
    SupconLayout v{};
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t at = off;
        off += align_up(bytes, 256);
        return at;
    };
    v.s2 = take((size_t)2 * B * B * sizeof(float));   // S, then S^T
    v.rmax = take((size_t)2 * B * sizeof(float));
    v.rlog = take((size_t)2 * B * sizeof(float));
    v.rinv = take((size_t)2 * B * sizeof(float));
    v.term = take((size_t)2 * B * sizeof(float));
    v.total = off;
    return v;
}

// ---------------------------------------------------------------------------------------------------------------------
// out[s][t][e] = sum over b ascending with idx[b] == s of src[b][tok0 + t][e]; V = 4: four consecutive e per thread
// ---------------------------------------------------------------------------------------------------------------------
template <int V>
__global__ __launch_bounds__(256) void rows_segment_sum_kernel(const float *__restrict__ src, const int64_t *__restrict__ idx,
                                                               int batch, int64_t prompt_stride, int64_t win0, int win,
                                                               float *__restrict__ out) {
    const int i = (blockIdx.y * 256 + threadIdx.x) * V;   // position inside the [n_tok][width] window
    if (i >= win) return;
    const int64_t s = blockIdx.x;
    float acc[V];
#pragma unroll
    for (int c = 0; c < V; ++c) acc[c] = 0.f;
    for (int b = 0; b < batch; ++b) {
        if (idx[b] != s) continue;
        const float *p = src + b * prompt_stride + win0 + i;
        if (V == 4) {
            const float4 x = *reinterpret_cast<const float4 *>(p);
            acc[0] += x.x;
            acc[1 % V] += x.y;
            acc[2 % V] += x.z;
            acc[3 % V] += x.w;
        } else {
            acc[0] += p[0];
        }
    }
    float *o = out + s * win + i;
    if (V == 4)
        *reinterpret_cast<float4 *>(o) = make_float4(acc[0], acc[1 % V], acc[2 % V], acc[3 % V]);
    else
        o[0] = acc[0];
}

// ---------------------------------------------------------------------------------------------------------------------
// Adam / AdamW
// ---------------------------------------------------------------------------------------------------------------------
struct AdamArgs {
    float w1, beta2, w2, a, r, eps, wd, lw;
    int decoupled;
};

__device__ __forceinline__ void adam_one(float &p, float g, float &m, float &v, const AdamArgs &c) {
    if (c.decoupled)
        p = fmaf(-c.lw, p, p);   // (not p * (1 - lw): rounding 1 - lw to fp32 alone costs half an ulp of p)
    else
        g = fmaf(c.wd, p, g);
    m = fmaf(c.w1, g - m, m);
    v = fmaf(c.w2, g * g, c.beta2 * v);
    p = fmaf(-c.a, __fdiv_rn(m, __fdiv_rn(sqrtf(v), c.r) + c.eps), p);
}

// threads 0 .. n4 - 1 take four elements each, the next n - 4 * n4 threads one element each behind them
__global__ __launch_bounds__(256) void adam_step_kernel(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m,
                                                        float *__restrict__ v, int64_t n4, int64_t n, AdamArgs c) {
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gid < n4) {
        float4 pp = reinterpret_cast<float4 *>(p)[gid], mm = reinterpret_cast<float4 *>(m)[gid], vv = reinterpret_cast<float4 *>(v)[gid];
        const float4 gg = reinterpret_cast<const float4 *>(g)[gid];
        adam_one(pp.x, gg.x, mm.x, vv.x, c);
        adam_one(pp.y, gg.y, mm.y, vv.y, c);
        adam_one(pp.z, gg.z, mm.z, vv.z, c);
        adam_one(pp.w, gg.w, mm.w, vv.w, c);
        reinterpret_cast<float4 *>(p)[gid] = pp;
        reinterpret_cast<float4 *>(m)[gid] = mm;
        reinterpret_cast<float4 *>(v)[gid] = vv;
        return;
    }
    const int64_t i = 4 * n4 + (gid - n4);
    if (i < n) adam_one(p[i], g[i], m[i], v[i], c);
}

}   // namespace

extern "C" size_t mpreid_supcon_workspace_bytes(int batch, int dim) {
    if (batch < 1 || batch > MPREID_SUPCON_MAX_BATCH || dim < 1) return 0;
    return supcon_layout(batch).total;
}

extern "C" int mpreid_supcon_f32(const float *img, const float *txt, const int64_t *labels, int B, int D, int dirs, float *loss,
                                 float *d_txt, float *d_img, void *ws, size_t ws_bytes, mpreid_stream_t stream_) {
    ARG_CHECK(img && txt && labels && loss && B >= 1 && D >= 1 && dirs >= 1 && dirs <= 3);
    if (B > MPREID_SUPCON_MAX_BATCH) {
        mpreid_set_error("supcon: batch %d above MPREID_SUPCON_MAX_BATCH = %d", B, MPREID_SUPCON_MAX_BATCH);
        return MPREID_ERR_UNSUPPORTED;
    }
    ARG_CHECK((((uintptr_t)img | (uintptr_t)txt | (uintptr_t)loss | (uintptr_t)d_txt | (uintptr_t)d_img) & 3) == 0 &&
              ((uintptr_t)labels & 7) == 0);
    const SupconLayout v = supcon_layout(B);
    if (!ws || ws_bytes < v.total) {
        mpreid_set_error("supcon workspace too small: %zu < %zu", ws_bytes, v.total);
        return MPREID_ERR_WORKSPACE;
    }
    ARG_CHECK(((uintptr_t)ws & 255) == 0);
    hipStream_t stream = (hipStream_t)stream_;
    char *base = (char *)ws;
    float *S2 = (float *)(base + v.s2);
    float *rmax = (float *)(base + v.rmax), *rlog = (float *)(base + v.rlog), *rinv = (float *)(base + v.rinv);
    float *term = (float *)(base + v.term);
    const unsigned tiles = (unsigned)((B + SC_T - 1) / SC_T);
    hipLaunchKernelGGL(supcon_logits_kernel, dim3(tiles, tiles), dim3(SC_T * SC_T), 0, stream, img, txt, B, D, S2,
                       S2 + (size_t)B * B);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(supcon_stats_kernel, dim3((unsigned)((2 * B + 3) / 4)), dim3(256), 0, stream, S2, labels, B, rmax, rlog, rinv,
                       term);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(supcon_loss_kernel, dim3(1), dim3(256), 0, stream, term, B, loss);
    LAUNCH_CHECK();
    if (d_img || d_txt) {
        const int side0 = d_img ? 0 : 1, sides = (d_img && d_txt) ? 2 : 1;
        hipLaunchKernelGGL(supcon_grad_kernel, dim3((unsigned)B, (unsigned)sides), dim3(256), 0, stream, S2, labels, rmax, rlog, rinv,
                           img, txt, B, D, side0, dirs, d_img, d_txt);
        LAUNCH_CHECK();
    }
    return MPREID_OK;
}

extern "C" int mpreid_supcon_pair_f32(const float *img, const float *txt, const int64_t *labels, int B, int D, float *loss,
                                      float *d_txt, float *d_img, void *ws, size_t ws_bytes, mpreid_stream_t stream) {
    return mpreid_supcon_f32(img, txt, labels, B, D, 3, loss, d_txt, d_img, ws, ws_bytes, stream);
}

extern "C" int mpreid_rows_segment_sum_f32(const float *src, const int64_t *idx, int batch, int tokens, int width, int tok0,
                                           int n_tok, int n_seg, float *out, mpreid_stream_t stream) {
    ARG_CHECK(src && idx && out && batch >= 1 && tokens >= 1 && width >= 1 && n_seg >= 1);
    ARG_CHECK(tok0 >= 0 && n_tok >= 1 && (int64_t)tok0 + n_tok <= tokens);
    ARG_CHECK((int64_t)n_tok * width < (int64_t)1 << 24 && (int64_t)batch * tokens * width < (int64_t)1 << 40);
    ARG_CHECK((((uintptr_t)src | (uintptr_t)out) & 3) == 0 && ((uintptr_t)idx & 7) == 0);
    const int win = n_tok * width;
    const int64_t stride = (int64_t)tokens * width, win0 = (int64_t)tok0 * width;
    if (width % 4 == 0 && (((uintptr_t)src | (uintptr_t)out) & 15) == 0) {
        hipLaunchKernelGGL(rows_segment_sum_kernel<4>, dim3((unsigned)n_seg, (unsigned)((win / 4 + 255) / 256)), dim3(256), 0,
                           (hipStream_t)stream, src, idx, batch, stride, win0, win, out);
    } else {
        hipLaunchKernelGGL(rows_segment_sum_kernel<1>, dim3((unsigned)n_seg, (unsigned)((win + 255) / 256)), dim3(256), 0,
                           (hipStream_t)stream, src, idx, batch, stride, win0, win, out);
    }
    LAUNCH_CHECK();
    return MPREID_OK;
}

extern "C" int mpreid_adam_step_f32(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n, int step,
                                    float lr, float beta1, float beta2, float eps, float weight_decay, int decoupled,
                                    mpreid_stream_t stream) {
    ARG_CHECK(param && grad && exp_avg && exp_avg_sq && n >= 1 && step >= 1);
    ARG_CHECK(n < (int64_t)1 << 38);   // (the grid: at most 2^30 workgroups)
    ARG_CHECK(std::isfinite(lr) && lr >= 0.f && std::isfinite(weight_decay) && weight_decay >= 0.f);
    ARG_CHECK(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f && std::isfinite(eps) && eps > 0.f);
    const uintptr_t all = (uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq;
    ARG_CHECK((all & 3) == 0);
    AdamArgs c;
    c.w1 = (float)(1.0 - (double)beta1);
    c.beta2 = beta2;
    c.w2 = (float)(1.0 - (double)beta2);
    c.a = (float)((double)lr / (1.0 - std::pow((double)beta1, (double)step)));
    c.r = (float)std::sqrt(1.0 - std::pow((double)beta2, (double)step));
    c.eps = eps;
    c.wd = weight_decay;
    c.lw = (float)((double)lr * (double)weight_decay);
    c.decoupled = decoupled != 0;
    const int64_t n4 = (all & 15) == 0 ? n / 4 : 0;
    const int64_t threads = n4 + (n - 4 * n4);
    hipLaunchKernelGGL(adam_step_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, param, grad,
                       exp_avg, exp_avg_sq, n4, n, c);
    LAUNCH_CHECK();
    return MPREID_OK;
}
