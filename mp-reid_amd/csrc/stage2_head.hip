// stage2_head.hip — the stage-2 head (include/mpreid.h): everything between the tower's three output features and the scalar
// loss of loss/make_loss.py, with the gradients back to those features and to the head's own parameters.  Row cross-entropy with
// label smoothing, the batch-hard triplet loss, BatchNorm1d in training mode (forward and backward) and the three small matrix
// products of a bias-free nn.Linear.  fp32 throughout, no atomics, every sum in a fixed order: the same bits from run to run.
// The kernels are small and latency-bound (batch 64); what counts is the number of launches.  A whole head step
// (mpreid.ops.Stage2Head.step) is
//   16 launches in the Uni-Prompt stage-2 form: identity branch 7 (BatchNorm forward, scores, cross-entropy 2, d_scores . W,
//      d_scores^T . y, BatchNorm backward), triplet 4 (distances, mining, loss, gradient), image-to-text 4 (logits,
//      cross-entropy 2, d_logits . text), and 1 for the total;
//   31 launches in the list form of make_loss with text features: two identity branches (14), three triplet losses (12), the
//      image-to-text branch (4) and the total (1); 27 without text features.
#include "common.h"

#include <cmath>

namespace {

// thread t of 256 holds a partial sum: butterfly per wave, then the four wave sums in order -> every thread gets the total
__device__ __forceinline__ float block_sum_256(float s, float *red /* [4] */) {
    s = wave_bfly_add(s);
    __syncthreads();   // (red may still be read from the previous call)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// out[0] = mul * sum of term[0 .. n - 1]: thread t of 256 adds the terms t, t + 256, ... ascending, then block_sum_256
__global__ __launch_bounds__(256) void sum_scaled_kernel(const float *__restrict__ term, int n, float mul, float *__restrict__ out) {
    __shared__ float red[4];
    float s = 0.f;
    for (int j = threadIdx.x; j < n; j += 256) s += term[j];
    s = block_sum_256(s, red);
    if (threadIdx.x == 0) out[0] = mul * s;
}

// ---------------------------------------------------------------------------------------------------------------------
// Row cross-entropy with label smoothing: one workgroup per row
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void xent_rows_kernel(const float *__restrict__ logits, int64_t ld, const int64_t *__restrict__ labels,
                                                        int K, float eps, float mul /* scale / rows */, float *__restrict__ row_loss,
                                                        float *__restrict__ d_logits, int *__restrict__ argmax) {
    __shared__ float red[4];
    __shared__ float wm[4];
    __shared__ int wi[4];
    const int tid = threadIdx.x, r = blockIdx.x;
    const float *row = logits + (int64_t)r * ld;
    // the maximum and its lowest index
    float m = -INFINITY;
    int mi = 0x7fffffff;
    for (int c = tid; c < K; c += 256) {
        const float x = row[c];
        if (x > m || (x == m && c < mi)) {
            m = x;
            mi = c;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float om = __shfl_xor(m, off, 64);
        const int oi = __shfl_xor(mi, off, 64);
        if (om > m || (om == m && oi < mi)) {
            m = om;
            mi = oi;
        }
    }
    if ((tid & 63) == 0) {
        wm[tid >> 6] = m;
        wi[tid >> 6] = mi;
    }
    __syncthreads();
    m = wm[0];
    mi = wi[0];
#pragma unroll
    for (int w = 1; w < 4; ++w)
        if (wm[w] > m || (wm[w] == m && wi[w] < mi)) {
            m = wm[w];
            mi = wi[w];
        }
    // sum of exp(x - max) over every class but the maximum's own (whose term is exactly 1), and of (x - max) over all
    float se = 0.f, sx = 0.f;
    for (int c = tid; c < K; c += 256) {
        const float z = row[c] - m;
        if (c != mi) se += expf(z);
        sx += z;
    }
    se = block_sum_256(se, red);
    sx = block_sum_256(sx, red);
    const float lg = log1pf(se);   // log sum_c exp(x_c - max): no digits lost where one class holds all the probability
    const int64_t y = labels[r];
    const bool has = y >= 0 && y < (int64_t)K;   // (a label is data: looked at before it is used as an address)
    const float fk = (float)K;
    const float t_off = __fdiv_rn(eps, fk);                 // eps / K
    const float omt = eps * __fdiv_rn(fk - 1.0f, fk);       // 1 - the target of the label's class: exactly 0 at K = 1
    const float t_hot = 1.0f - omt;
    if (tid == 0) {
        const float hot = has ? (1.0f - eps) * (lg - (row[y] - m)) : 0.f;
        row_loss[r] = hot + t_off * (fk * lg - sx);
        if (argmax) argmax[r] = mi;
    }
    if (d_logits) {
        float *out = d_logits + (int64_t)r * K;
        const float q = __fdiv_rn(se, 1.0f + se);   // 1 - p of the maximum's class
        for (int c = tid; c < K; c += 256) {
            const bool lab = has && c == (int)y;
            float v;
            if (c == mi)
                v = lab ? omt - q : (1.0f - q) - t_off;   // (p - t without the cancellation of p = 1 - q against t = 1 - omt)
            else
                v = expf((row[c] - m) - lg) - (lab ? t_hot : t_off);
            out[c] = mul * v;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Batch-hard triplet loss
// ---------------------------------------------------------------------------------------------------------------------
constexpr int TR_T = 16, TR_K = 32;

// d2_ab = sum_e (x_ae - x_be)^2, ONE fmaf chain over the features ascending; a 16 x 16 tile per workgroup
__global__ __launch_bounds__(TR_T * TR_T) void triplet_dist_kernel(const float *__restrict__ x, int B, int D, float *__restrict__ d2) {
    __shared__ float As[TR_T][TR_K + 1], Bs[TR_T][TR_K + 1];
    const int tx = threadIdx.x & (TR_T - 1), ty = threadIdx.x / TR_T;
    const int a0 = blockIdx.y * TR_T, b0 = blockIdx.x * TR_T;
    float acc = 0.f;
    for (int k0 = 0; k0 < D; k0 += TR_K) {
        for (int i = threadIdx.x; i < TR_T * TR_K; i += TR_T * TR_T) {
            const int r = i / TR_K, c = i - r * TR_K;
            const bool kin = k0 + c < D;
            As[r][c] = (kin && a0 + r < B) ? x[(int64_t)(a0 + r) * D + k0 + c] : 0.f;
            Bs[r][c] = (kin && b0 + r < B) ? x[(int64_t)(b0 + r) * D + k0 + c] : 0.f;
        }
        __syncthreads();
        const int kn = min(TR_K, D - k0);
        for (int c = 0; c < kn; ++c) {
            const float df = As[ty][c] - Bs[tx][c];
            acc = fmaf(df, df, acc);
        }
        __syncthreads();
    }
    const int a = a0 + ty, b = b0 + tx;
    if (a < B && b < B) d2[(int64_t)a * B + b] = acc;
}

constexpr float TR_CLAMP = 1e-12f;

// One wave per anchor: the hardest positive (largest d, lowest index) and the hardest negative (smallest d, lowest index), the
// anchor's loss term, and the two coefficients of its gradient terms (0 where a term contributes nothing).
__global__ __launch_bounds__(256) void triplet_mine_kernel(const float *__restrict__ d2, const int64_t *__restrict__ labels, int B,
                                                           float margin, int soft, float hard_factor, float mul /* scale / B */,
                                                           float *__restrict__ dist_ap, float *__restrict__ dist_an,
                                                           int *__restrict__ p_idx, int *__restrict__ n_idx, float *__restrict__ term,
                                                           float *__restrict__ cp, float *__restrict__ cn) {
    const int lane = threadIdx.x & 63;
    const int a = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (a >= B) return;
    const float *row = d2 + (int64_t)a * B;
    const int64_t mine = labels[a];
    float dp = -INFINITY, dn = INFINITY;
    int ip = 0x7fffffff, in = 0x7fffffff;
    for (int j = lane; j < B; j += 64) {
        const float d = sqrtf(fmaxf(row[j], TR_CLAMP));
        if (labels[j] == mine) {
            if (d > dp || (d == dp && j < ip)) {
                dp = d;
                ip = j;
            }
        } else if (d < dn || (d == dn && j < in)) {
            dn = d;
            in = j;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float op = __shfl_xor(dp, off, 64), on = __shfl_xor(dn, off, 64);
        const int jp = __shfl_xor(ip, off, 64), jn = __shfl_xor(in, off, 64);
        if (op > dp || (op == dp && jp < ip)) {
            dp = op;
            ip = jp;
        }
        if (on < dn || (on == dn && jn < in)) {
            dn = on;
            in = jn;
        }
    }
    if (lane != 0) return;
    // (the anchor itself is a positive: ip is always a row)
    const float fp = 1.0f + hard_factor, fn = 1.0f - hard_factor;
    const float ap = dp * fp;
    const bool has_n = in != 0x7fffffff;
    dist_ap[a] = ap;
    p_idx[a] = ip;
    if (!has_n) {
        dist_an[a] = INFINITY;
        n_idx[a] = -1;
        term[a] = 0.f;
        cp[a] = 0.f;
        cn[a] = 0.f;
        return;
    }
    const float an = dn * fn;
    dist_an[a] = an;
    n_idx[a] = in;
    float per, w;
    if (soft) {
        const float z = ap - an, e = expf(-fabsf(z));   // log(1 + exp(z)) = max(z, 0) + log1p(exp(-|z|)): no overflow
        per = fmaxf(z, 0.f) + log1pf(e);
        w = z >= 0.f ? __fdiv_rn(1.0f, 1.0f + e) : __fdiv_rn(e, 1.0f + e);
    } else {
        const float z = (ap - an) + margin;
        per = fmaxf(z, 0.f);
        w = z > 0.f ? 1.f : 0.f;
    }
    term[a] = per;
    const float g = mul * w;
    cp[a] = row[ip] >= TR_CLAMP ? __fdiv_rn(g * fp, dp) : 0.f;   // (a pair below the clamp: the clamp's gradient is 0)
    cn[a] = row[in] >= TR_CLAMP ? __fdiv_rn(g * fn, dn) : 0.f;
}

// d_feat row r, one workgroup: the anchors in ascending order; for each of them what r receives as the anchor itself (its
// positive term, then its negative term), then as its positive, then as its negative.  One fmaf per term.
__global__ __launch_bounds__(256) void triplet_grad_kernel(const float *__restrict__ x, int B, int D, const int *__restrict__ p_idx,
                                                           const int *__restrict__ n_idx, const float *__restrict__ cp,
                                                           const float *__restrict__ cn, float *__restrict__ d_feat) {
    __shared__ int sa[3 * 1024 + 4];     // the list of (anchor, role) pairs that touch r, in the fixed order
    __shared__ int cnt;
    const int r = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) {
        int n = 0;
        for (int a = 0; a < B; ++a) {
            const int p = p_idx[a], q = n_idx[a];
            if (a == r) {
                if (cp[a] != 0.f) sa[n++] = a * 4 + 0;
                if (cn[a] != 0.f) sa[n++] = a * 4 + 1;
            }
            if (p == r && cp[a] != 0.f) sa[n++] = a * 4 + 2;
            if (q == r && cn[a] != 0.f) sa[n++] = a * 4 + 3;
        }
        cnt = n;
    }
    __syncthreads();
    const int n = cnt;
    const float *xr = x + (int64_t)r * D;
    for (int e = tid; e < D; e += 256) {
        const float v = xr[e];
        float acc = 0.f;
        for (int i = 0; i < n; ++i) {
            const int a = sa[i] >> 2, role = sa[i] & 3;
            if (role == 0)
                acc = fmaf(cp[a], v - x[(int64_t)p_idx[a] * D + e], acc);
            else if (role == 1)
                acc = fmaf(-cn[a], v - x[(int64_t)n_idx[a] * D + e], acc);
            else if (role == 2)
                acc = fmaf(-cp[a], x[(int64_t)a * D + e] - v, acc);
            else
                acc = fmaf(cn[a], x[(int64_t)a * D + e] - v, acc);
        }
        d_feat[(int64_t)r * D + e] = acc;
    }
}

struct TripletLayout {
    size_t d2, term, cp, cn, total;
};

TripletLayout triplet_layout(int B) {
    TripletLayout v{};
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t at = off;
        off += align_up(bytes, 256);
        return at;
    };
    v.d2 = take((size_t)B * B * sizeof(float));
    v.term = take((size_t)B * sizeof(float));
    v.cp = take((size_t)B * sizeof(float));
    v.cn = take((size_t)B * sizeof(float));
    v.total = off;
    return v;
}

// ---------------------------------------------------------------------------------------------------------------------
// BatchNorm1d in training mode: one thread per column, rows ascending
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void bn1d_forward_kernel(const float *__restrict__ x, const float *__restrict__ gamma,
                                                          const float *__restrict__ beta, int B, int D, float eps, float momentum,
                                                          float *__restrict__ y, float *__restrict__ mean, float *__restrict__ invstd,
                                                          float *__restrict__ running_mean, float *__restrict__ running_var) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= D) return;
    const float fb = (float)B;
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += x[(int64_t)b * D + e];
    const float mu = __fdiv_rn(s, fb);
    float q = 0.f;
    for (int b = 0; b < B; ++b) {
        const float c = x[(int64_t)b * D + e] - mu;
        q = fmaf(c, c, q);
    }
    const float var = __fdiv_rn(q, fb);
    const float inv = __fdiv_rn(1.0f, sqrtf(var + eps));
    const float g = gamma[e], bt = beta[e];
    for (int b = 0; b < B; ++b) y[(int64_t)b * D + e] = fmaf((x[(int64_t)b * D + e] - mu) * inv, g, bt);
    mean[e] = mu;
    invstd[e] = inv;
    if (running_mean) {
        running_mean[e] = fmaf(momentum, mu - running_mean[e], running_mean[e]);
        const float unb = __fdiv_rn(q, fb - 1.0f);
        running_var[e] = fmaf(momentum, unb - running_var[e], running_var[e]);
    }
}

__global__ __launch_bounds__(64) void bn1d_backward_kernel(const float *__restrict__ x, const float *__restrict__ dy,
                                                           const float *__restrict__ gamma, const float *__restrict__ mean,
                                                           const float *__restrict__ invstd, const float *__restrict__ dx_add, int B,
                                                           int D, float *__restrict__ dx, float *__restrict__ dgamma,
                                                           float *__restrict__ dbeta) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= D) return;
    const float mu = mean[e], inv = invstd[e], fb = (float)B;
    float s1 = 0.f, s2 = 0.f;
    for (int b = 0; b < B; ++b) {
        const float g = dy[(int64_t)b * D + e];
        s1 += g;
        s2 = fmaf(g, (x[(int64_t)b * D + e] - mu) * inv, s2);
    }
    const float k = __fdiv_rn(gamma[e] * inv, fb);
    for (int b = 0; b < B; ++b) {
        const float xh = (x[(int64_t)b * D + e] - mu) * inv;
        const float v = k * ((fb * dy[(int64_t)b * D + e] - s1) - xh * s2);
        dx[(int64_t)b * D + e] = dx_add ? v + dx_add[(int64_t)b * D + e] : v;
    }
    dgamma[e] = s2;
    if (dbeta) dbeta[e] = s1;
}

// ---------------------------------------------------------------------------------------------------------------------
// C[m][n] = sum_k A(m, k) B(n, k), A(m, k) = a[m * a_rs + k * a_cs], B(n, k) = b[n * b_rs + k * b_cs]: a 16 x 16 tile of C per
// workgroup, one element per thread, ONE fmaf chain over k ascending (then + c_add[m][n], when given).  The tile loads walk
// whichever index has stride 1.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int MM_T = 16, MM_K = 32;

__global__ __launch_bounds__(MM_T * MM_T) void matmul_f32_kernel(const float *__restrict__ a, int64_t a_rs, int64_t a_cs,
                                                                 const float *__restrict__ b, int64_t b_rs, int64_t b_cs, int M, int N,
                                                                 int K, const float *__restrict__ c_add, float *__restrict__ c, int64_t ldc) {
    __shared__ float As[MM_T][MM_K + 1], Bs[MM_T][MM_K + 1];
    const int tx = threadIdx.x & (MM_T - 1), ty = threadIdx.x / MM_T;
    const int m0 = blockIdx.y * MM_T, n0 = blockIdx.x * MM_T;
    float acc = 0.f;
    for (int k0 = 0; k0 < K; k0 += MM_K) {
        for (int i = threadIdx.x; i < MM_T * MM_K; i += MM_T * MM_T) {
            int r, cc;
            if (a_cs == 1) { r = i / MM_K; cc = i - r * MM_K; } else { cc = i / MM_T; r = i - cc * MM_T; }
            As[r][cc] = (k0 + cc < K && m0 + r < M) ? a[(int64_t)(m0 + r) * a_rs + (int64_t)(k0 + cc) * a_cs] : 0.f;
            if (b_cs == 1) { r = i / MM_K; cc = i - r * MM_K; } else { cc = i / MM_T; r = i - cc * MM_T; }
            Bs[r][cc] = (k0 + cc < K && n0 + r < N) ? b[(int64_t)(n0 + r) * b_rs + (int64_t)(k0 + cc) * b_cs] : 0.f;
        }
        __syncthreads();
        const int kn = min(MM_K, K - k0);
        for (int cc = 0; cc < kn; ++cc) acc = fmaf(As[ty][cc], Bs[tx][cc], acc);
        __syncthreads();
    }
    const int m = m0 + ty, n = n0 + tx;
    if (m < M && n < N) c[(int64_t)m * ldc + n] = c_add ? acc + c_add[(int64_t)m * ldc + n] : acc;
}

// out[0] = total, out[1] = identity part, out[2] = triplet part, out[3] = image-to-text part, from the terms in that order
__global__ void stage2_total_kernel(const float *__restrict__ terms, int n_id, int n_tri, int n_i2t, float *__restrict__ out) {
    if (threadIdx.x != 0) return;
    float id = 0.f, tri = 0.f, i2t = 0.f;
    int j = 0;
    for (int i = 0; i < n_id; ++i) id += terms[j++];
    for (int i = 0; i < n_tri; ++i) tri += terms[j++];
    for (int i = 0; i < n_i2t; ++i) i2t += terms[j++];
    out[0] = i2t + (id + tri);   // (make_loss: I2T_LOSS_WEIGHT * I2TLOSS + (ID_LOSS_WEIGHT * ID_LOSS + TRIPLET_LOSS_WEIGHT * TRI_LOSS))
    out[1] = id;
    out[2] = tri;
    out[3] = i2t;
}

inline bool aligned4(std::initializer_list<const void *> ps) {
    uintptr_t all = 0;
    for (const void *p : ps) all |= (uintptr_t)p;
    return (all & 3) == 0;
}

}   // namespace

extern "C" int mpreid_xent_rows_f32(const float *logits, int64_t ld, const int64_t *labels, int rows, int classes, float epsilon,
                                    float scale, float *loss, float *row_loss, float *d_logits, int32_t *argmax,
                                    mpreid_stream_t stream_) {
    ARG_CHECK(logits && labels && loss && row_loss && rows >= 1 && classes >= 1 && ld >= classes);
    ARG_CHECK(std::isfinite(epsilon) && epsilon >= 0.f && epsilon <= 1.f && std::isfinite(scale));
    ARG_CHECK(aligned4({logits, loss, row_loss, d_logits, argmax}) && ((uintptr_t)labels & 7) == 0);
    ARG_CHECK((int64_t)rows * ld < (int64_t)1 << 40);
    hipStream_t stream = (hipStream_t)stream_;
    const float mul = (float)((double)scale / (double)rows);
    hipLaunchKernelGGL(xent_rows_kernel, dim3((unsigned)rows), dim3(256), 0, stream, logits, ld, labels, classes, epsilon, mul,
                       row_loss, d_logits, (int *)argmax);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(sum_scaled_kernel, dim3(1), dim3(256), 0, stream, (const float *)row_loss, rows, mul, loss);
    LAUNCH_CHECK();
    return MPREID_OK;
}

extern "C" size_t mpreid_triplet_workspace_bytes(int batch, int dim) {
    if (batch < 1 || batch > MPREID_TRIPLET_MAX_BATCH || dim < 1) return 0;
    return triplet_layout(batch).total;
}

extern "C" int mpreid_triplet_hard_f32(const float *feat, const int64_t *labels, int B, int D, float margin, int soft_margin,
                                       float hard_factor, float scale, float *loss, float *dist_ap, float *dist_an, int32_t *p_idx,
                                       int32_t *n_idx, float *d_feat, void *ws, size_t ws_bytes, mpreid_stream_t stream_) {
    ARG_CHECK(feat && labels && loss && dist_ap && dist_an && p_idx && n_idx && B >= 1 && D >= 1);
    if (B > MPREID_TRIPLET_MAX_BATCH) {
        mpreid_set_error("triplet: batch %d above MPREID_TRIPLET_MAX_BATCH = %d", B, MPREID_TRIPLET_MAX_BATCH);
        return MPREID_ERR_UNSUPPORTED;
    }
    ARG_CHECK(std::isfinite(margin) && std::isfinite(hard_factor) && std::isfinite(scale));
    ARG_CHECK(aligned4({feat, loss, dist_ap, dist_an, p_idx, n_idx, d_feat}) && ((uintptr_t)labels & 7) == 0);
    const TripletLayout v = triplet_layout(B);
    if (!ws || ws_bytes < v.total) {
        mpreid_set_error("triplet workspace too small: %zu < %zu", ws_bytes, v.total);
        return MPREID_ERR_WORKSPACE;
    }
    ARG_CHECK(((uintptr_t)ws & 255) == 0);
    hipStream_t stream = (hipStream_t)stream_;
    char *base = (char *)ws;
    float *d2 = (float *)(base + v.d2), *term = (float *)(base + v.term), *cp = (float *)(base + v.cp), *cn = (float *)(base + v.cn);
    const float mul = (float)((double)scale / (double)B);
    const unsigned tiles = (unsigned)((B + TR_T - 1) / TR_T);
    hipLaunchKernelGGL(triplet_dist_kernel, dim3(tiles, tiles), dim3(TR_T * TR_T), 0, stream, feat, B, D, d2);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(triplet_mine_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, stream, (const float *)d2, labels, B, margin,
                       soft_margin != 0 ? 1 : 0, hard_factor, mul, dist_ap, dist_an, (int *)p_idx, (int *)n_idx, term, cp, cn);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(sum_scaled_kernel, dim3(1), dim3(256), 0, stream, (const float *)term, B, mul, loss);
    LAUNCH_CHECK();
    if (d_feat) {
        hipLaunchKernelGGL(triplet_grad_kernel, dim3((unsigned)B), dim3(256), 0, stream, feat, B, D, (const int *)p_idx,
                           (const int *)n_idx, (const float *)cp, (const float *)cn, d_feat);
        LAUNCH_CHECK();
    }
    return MPREID_OK;
}

extern "C" int mpreid_bn1d_train_forward_f32(const float *x, const float *gamma, const float *beta, int B, int D, float eps,
                                             float momentum, float *y, float *mean, float *invstd, float *running_mean,
                                             float *running_var, mpreid_stream_t stream) {
    ARG_CHECK(x && gamma && beta && y && mean && invstd && D >= 1 && B >= 1);
    if (B < 2) {
        mpreid_set_error("bn1d_train: a batch of %d has no variance (torch refuses it in training mode as well)", B);
        return MPREID_ERR_ARG;
    }
    ARG_CHECK((running_mean != nullptr) == (running_var != nullptr));
    ARG_CHECK(std::isfinite(eps) && eps > 0.f && std::isfinite(momentum) && momentum >= 0.f && momentum <= 1.f);
    ARG_CHECK(aligned4({x, gamma, beta, y, mean, invstd, running_mean, running_var}));
    ARG_CHECK((int64_t)B * D < (int64_t)1 << 40);
    hipLaunchKernelGGL(bn1d_forward_kernel, dim3((unsigned)((D + 63) / 64)), dim3(64), 0, (hipStream_t)stream, x, gamma, beta, B, D, eps,
                       momentum, y, mean, invstd, running_mean, running_var);
    LAUNCH_CHECK();
    return MPREID_OK;
}

extern "C" int mpreid_bn1d_train_backward_f32(const float *x, const float *dy, const float *gamma, const float *mean,
                                              const float *invstd, const float *dx_add, int B, int D, float *dx, float *dgamma,
                                              float *dbeta, mpreid_stream_t stream) {
    ARG_CHECK(x && dy && gamma && mean && invstd && dx && dgamma && D >= 1 && B >= 2);
    ARG_CHECK(aligned4({x, dy, gamma, mean, invstd, dx_add, dx, dgamma, dbeta}));
    ARG_CHECK((int64_t)B * D < (int64_t)1 << 40);
    hipLaunchKernelGGL(bn1d_backward_kernel, dim3((unsigned)((D + 63) / 64)), dim3(64), 0, (hipStream_t)stream, x, dy, gamma, mean,
                       invstd, dx_add, B, D, dx, dgamma, dbeta);
    LAUNCH_CHECK();
    return MPREID_OK;
}

extern "C" int mpreid_matmul_f32(const float *a, int64_t a_rs, int64_t a_cs, const float *b, int64_t b_rs, int64_t b_cs, int M, int N,
                                 int K, const float *c_add, float *c, int64_t ldc, mpreid_stream_t stream) {
    ARG_CHECK(a && b && c && M >= 1 && N >= 1 && K >= 1 && ldc >= N);
    ARG_CHECK(a_rs >= 1 && a_cs >= 1 && b_rs >= 1 && b_cs >= 1);
    ARG_CHECK(aligned4({a, b, c, c_add}));
    const int64_t lim = (int64_t)1 << 40;
    ARG_CHECK((M - 1) * a_rs + (K - 1) * a_cs < lim && (N - 1) * b_rs + (K - 1) * b_cs < lim && (int64_t)M * ldc < lim);
    ARG_CHECK((M + MM_T - 1) / MM_T <= 65535);
    hipLaunchKernelGGL(matmul_f32_kernel, dim3((unsigned)((N + MM_T - 1) / MM_T), (unsigned)((M + MM_T - 1) / MM_T)), dim3(MM_T * MM_T), 0,
                       (hipStream_t)stream, a, a_rs, a_cs, b, b_rs, b_cs, M, N, K, c_add, c, ldc);
    LAUNCH_CHECK();
    return MPREID_OK;
}

extern "C" int mpreid_stage2_total_f32(const float *terms, int n_id, int n_tri, int n_i2t, float *out, mpreid_stream_t stream) {
    ARG_CHECK(terms && out && n_id >= 0 && n_tri >= 0 && n_i2t >= 0 && n_id + n_tri + n_i2t >= 1 && n_id + n_tri + n_i2t <= 64);
    ARG_CHECK(aligned4({terms, out}));
    hipLaunchKernelGGL(stage2_total_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, terms, n_id, n_tri, n_i2t, out);
    LAUNCH_CHECK();
    return MPREID_OK;
}
