// text_grad.hip — mpreid_text_backward: the gradient of the text features with respect to the prompts, every tower weight
// frozen (include/mpreid.h).  The call re-runs the forward's own blocks (csrc/vit.hip through towers.h), keeps each
// block's input, and walks the layers back through the one differentiation of a block (block_mlp_backward /
// block_attention_backward, csrc/vit_grad.hip) with no parameter gradient asked for: per layer q | k | v, the block's
// mid-point and the FC1 pre-activation are recomputed with the forward's launchers, and the gradient is propagated with the
// exact fp32 GEMM over transposed fp32 weights (dX = dY . W) and the fp32 kernels below, which the image tower's sweep
// launches as well (all but the causal attention gradient).  No weight gradient, no atomics: the same bits from run to run.
#include "towers.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// causal attention backward: one workgroup per (prompt, head), Q, K, V and dO of the head in LDS
// ---------------------------------------------------------------------------------------------------------------------
constexpr int AB_NW = 8;     // waves per workgroup
constexpr int AB_LD = 68;    // floats per LDS row: 64 + 4, so that the 16-byte reads of 16 consecutive rows cover all 64 banks
constexpr int AB_MAXL = MPREID_TEXT_MAX_TOKENS;

static size_t attn_bwd_lds_bytes(int L) { return ((size_t)4 * L * AB_LD + 4 * AB_MAXL + AB_NW * 2 * AB_MAXL) * sizeof(float); }

// qkv [B * L][3W] (q | k | v, head h in columns h * 64 ..), d_o [B * L][W] -> d_qkv [B * L][3W].
// P = softmax(mask(q k^T / 8)), dV = P^T dO, dP = dO V^T, dS = P o (dP - rowsum(P o dP)), dQ = dS K / 8, dK = dS^T Q / 8.
// Phase 1, a wave per query row i (lane = key): the row's max, sum and rowsum(P o dP) -> LDS; dS of the row -> the wave's
// LDS strip; then lane = feature: dQ[i].  Phase 2, a wave per key j (lane = query): P and dS of the column from the stored row
// statistics -> the strip; then lane = feature: dK[j], dV[j], summed over the query rows i >= j in ascending order inside the
// wave.  Keys behind the query (j > i) are never read: they contribute exactly nothing.
// dS is taken about the row's strongest key j*: with r = dP[i][j*], dS = P o ((dP - r) - rowsum(P o (dP - r))), the same value
// in exact arithmetic (P sums to one).  In a saturated row, P[i][j*] -> 1, the plain form subtracts two nearly equal numbers
// and loses log2(1 / (1 - P[i][j*])) bits of dS[i][j*] -- which is all there is of dQ and dK when the row is the slab (two
// tokens); about r the term of j* in the row sum is exactly zero and nothing cancels.
__global__ __launch_bounds__(64 * AB_NW) void text_attention_backward_kernel(const float *__restrict__ qkv,
                                                                            const float *__restrict__ d_o, int L, int W,
                                                                            int heads, float *__restrict__ d_qkv) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *Qs = reinterpret_cast<float *>(smem);
    float *Ks = Qs + (size_t)L * AB_LD;
    float *Vs = Ks + (size_t)L * AB_LD;
    float *Gs = Vs + (size_t)L * AB_LD;
    float *row_max = Gs + (size_t)L * AB_LD;
    float *row_sum = row_max + AB_MAXL;
    float *row_ref = row_sum + AB_MAXL;
    float *row_dot = row_ref + AB_MAXL;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float *strip_p = row_dot + AB_MAXL + wave * 2 * AB_MAXL;   // (row_dot is the last of the four row arrays)
    float *strip_ds = strip_p + AB_MAXL;

    const int b = blockIdx.x / heads, h = blockIdx.x - b * heads;
    const int64_t row0 = (int64_t)b * L;
    for (int idx = tid; idx < L * 16; idx += 64 * AB_NW) {
        const int r = idx >> 4, c = (idx & 15) * 4;
        const float *src = qkv + (row0 + r) * 3 * W + h * 64 + c;
        *reinterpret_cast<float4 *>(Qs + r * AB_LD + c) = *reinterpret_cast<const float4 *>(src);
        *reinterpret_cast<float4 *>(Ks + r * AB_LD + c) = *reinterpret_cast<const float4 *>(src + W);
        *reinterpret_cast<float4 *>(Vs + r * AB_LD + c) = *reinterpret_cast<const float4 *>(src + 2 * W);
        *reinterpret_cast<float4 *>(Gs + r * AB_LD + c) = *reinterpret_cast<const float4 *>(d_o + (row0 + r) * W + h * 64 + c);
    }
    __syncthreads();

    for (int i = wave; i < L; i += AB_NW) {
        float s[2], dp[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int j = lane + 64 * t;
            s[t] = -INFINITY;
            dp[t] = 0.f;
            if (j <= i) {
                s[t] = dot64(Qs + i * AB_LD, Ks + j * AB_LD) * 0.125f;
                dp[t] = dot64(Gs + i * AB_LD, Vs + j * AB_LD);
            }
        }
        const float m = wave_bfly_max(fmaxf(s[0], s[1]));
        float e[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) e[t] = (lane + 64 * t <= i) ? expf(s[t] - m) : 0.f;
        const float sum = wave_bfly_add(e[0] + e[1]);
        const float p0 = __fdiv_rn(e[0], sum), p1 = __fdiv_rn(e[1], sum);
        // r = dP of the first key that holds the row's maximum (one lane contributes: the sum is that value exactly)
        int jstar = s[0] == m ? lane : (s[1] == m ? lane + 64 : AB_MAXL);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) jstar = min(jstar, __shfl_xor(jstar, off, 64));
        const float ref = wave_bfly_add(lane == jstar ? dp[0] : (lane + 64 == jstar ? dp[1] : 0.f));
        const float c0 = dp[0] - ref, c1 = dp[1] - ref;
        const float dot = wave_bfly_add(fmaf(p1, c1, p0 * c0));   // (p = 0 behind the query row)
        if (lane == 0) {
            row_max[i] = m;
            row_sum[i] = sum;
            row_ref[i] = ref;
            row_dot[i] = dot;
        }
        if (lane <= i) strip_ds[lane] = p0 * (c0 - dot);
        if (lane + 64 <= i) strip_ds[lane + 64] = p1 * (c1 - dot);
        wave_lds_sync();
        float acc = 0.f;
        for (int j = 0; j <= i; ++j) acc = fmaf(strip_ds[j], Ks[j * AB_LD + lane], acc);
        d_qkv[(row0 + i) * 3 * W + h * 64 + lane] = acc * 0.125f;
        wave_lds_sync();
    }
    __syncthreads();

    for (int j = wave; j < L; j += AB_NW) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int i = lane + 64 * t;
            if (i >= j && i < L) {
                const float sc = dot64(Qs + i * AB_LD, Ks + j * AB_LD) * 0.125f;
                const float p = __fdiv_rn(expf(sc - row_max[i]), row_sum[i]);
                const float dp = dot64(Gs + i * AB_LD, Vs + j * AB_LD);
                strip_p[i] = p;
                strip_ds[i] = p * ((dp - row_ref[i]) - row_dot[i]);
            }
        }
        wave_lds_sync();
        float dk = 0.f, dv = 0.f;
        for (int i = j; i < L; ++i) {
            dk = fmaf(strip_ds[i], Qs[i * AB_LD + lane], dk);
            dv = fmaf(strip_p[i], Gs[i * AB_LD + lane], dv);
        }
        float *dst = d_qkv + (row0 + j) * 3 * W + h * 64 + lane;
        dst[W] = dk * 0.125f;
        dst[2 * W] = dv;
        wave_lds_sync();
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// LayerNorm input gradient (biased variance, eps 1e-5, statistics recomputed from x; one wave per row):
// dx = (g o dy - mean(g o dy) - xhat * mean(g o dy o xhat)) / sigma;  ACC: dx is added to what `out` holds
// ---------------------------------------------------------------------------------------------------------------------
template <bool ACC>
__global__ __launch_bounds__(256) void layernorm_backward_kernel(const float *__restrict__ x, const float *__restrict__ dy,
                                                                 const float *__restrict__ g, int64_t rows, int W,
                                                                 float *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float *xr = x + row * W, *dr = dy + row * W;
    float *orow = out + row * W;
    float s = 0.f;
    for (int k = lane; k < W; k += 64) s += xr[k];
    const float mean = wave_bfly_add(s) / (float)W;
    float q = 0.f;
    for (int k = lane; k < W; k += 64) {
        const float d = xr[k] - mean;
        q = fmaf(d, d, q);
    }
    const float rstd = 1.0f / sqrtf(wave_bfly_add(q) / (float)W + 1e-5f);
    float s1 = 0.f, s2 = 0.f;
    for (int k = lane; k < W; k += 64) {
        const float a = g[k] * dr[k];
        s1 += a;
        s2 = fmaf(a, (xr[k] - mean) * rstd, s2);
    }
    const float c1 = wave_bfly_add(s1) / (float)W, c2 = wave_bfly_add(s2) / (float)W;
    for (int k = lane; k < W; k += 64) {
        const float v = ((g[k] * dr[k] - c1) - ((xr[k] - mean) * rstd) * c2) * rstd;
        orow[k] = ACC ? orow[k] + v : v;
    }
}

// QuickGELU backward, in place: d[i] = d[i] * (s + 1.702 u s (1 - s)), s = sigmoid(1.702 u); one float4 per thread
__global__ __launch_bounds__(256) void quickgelu_backward_kernel(const float *__restrict__ u, float *__restrict__ d, int64_t n4) {
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gid >= n4) return;
    const float4 uu = reinterpret_cast<const float4 *>(u)[gid];
    float4 dd = reinterpret_cast<float4 *>(d)[gid];
    auto slope = [](float t) {
        const float sg = __fdiv_rn(1.0f, 1.0f + expf(-1.702f * t));
        return fmaf(1.702f * t * sg, 1.0f - sg, sg);
    };
    dd.x *= slope(uu.x);
    dd.y *= slope(uu.y);
    dd.z *= slope(uu.z);
    dd.w *= slope(uu.w);
    reinterpret_cast<float4 *>(d)[gid] = dd;
}

// sum over the 256 threads of a workgroup, the same value in every thread: wave butterflies, then the four partials in order
__device__ __forceinline__ float block_sum(float v, float *red) {
    v = wave_bfly_add(v);
    __syncthreads();   // `red` of the previous sum has been read
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// The head, backwards, for prompt b = blockIdx.x: dy = grad_out[b] @ text_projection^T (proj_t: [out_dim][W]), ln_final's
// input gradient at the read-out row, written to row eot[b] of dx; every other row of the prompt is set to zero.  The row
// index is clamped into the prompt as in the forward (head_ln_kernel, csrc/vit.hip).
__global__ __launch_bounds__(256) void text_head_backward_kernel(const float *__restrict__ x, const int32_t *__restrict__ eot,
                                                                 const float *__restrict__ grad_out, int L, int W, int out_dim,
                                                                 const float *__restrict__ proj_t, const float *__restrict__ g,
                                                                 float *__restrict__ dx) {
    __shared__ float dy[1024];   // width <= 1024 (text_check_shape)
    __shared__ float red[4];
    const int tid = threadIdx.x, b = blockIdx.x;
    int e = eot[b];
    e = e < 0 ? 0 : (e > L - 1 ? L - 1 : e);
    const float *go = grad_out + (int64_t)b * out_dim;
    for (int k = tid; k < W; k += 256) {
        float acc = 0.f;
        for (int o = 0; o < out_dim; ++o) acc = fmaf(go[o], proj_t[(int64_t)o * W + k], acc);
        dy[k] = g[k] * acc;
    }
    const float *xr = x + ((int64_t)b * L + e) * W;
    float s = 0.f;
    for (int k = tid; k < W; k += 256) s += xr[k];
    const float mean = block_sum(s, red) / (float)W;
    float q = 0.f;
    for (int k = tid; k < W; k += 256) {
        const float d = xr[k] - mean;
        q = fmaf(d, d, q);
    }
    const float rstd = 1.0f / sqrtf(block_sum(q, red) / (float)W + 1e-5f);
    float s1 = 0.f, s2 = 0.f;
    for (int k = tid; k < W; k += 256) {   // (dy[k] was written by this very thread)
        s1 += dy[k];
        s2 = fmaf(dy[k], (xr[k] - mean) * rstd, s2);
    }
    const float c1 = block_sum(s1, red) / (float)W;
    const float c2 = block_sum(s2, red) / (float)W;
    float *dst = dx + (int64_t)b * L * W;
    for (int r = 0; r < L; ++r)
        for (int k = tid; k < W; k += 256)
            dst[(int64_t)r * W + k] = r == e ? ((dy[k] - c1) - ((xr[k] - mean) * rstd) * c2) * rstd : 0.f;
}

}   // namespace

// (towers.h: launched by the differentiation of a block, csrc/vit_grad.hip)
int launch_causal_attention_backward(const float *qkv, const float *d_o, int B, int L, int W, int heads, float *d_qkv,
                                     hipStream_t s) {
    const size_t lds = attn_bwd_lds_bytes(L);
    const int rc = mpreid_dyn_lds(text_attention_backward_kernel, lds);
    if (rc) return rc;
    hipLaunchKernelGGL(text_attention_backward_kernel, dim3((unsigned)(B * heads)), dim3(64 * AB_NW), lds, s, qkv, d_o, L, W, heads,
                       d_qkv);
    LAUNCH_CHECK();
    return MPREID_OK;
}

int launch_layernorm_backward(const float *x, const float *dy, const float *g, int64_t rows, int W, bool acc, float *out,
                              hipStream_t s) {
    const dim3 grid((unsigned)((rows + 3) / 4));
    if (acc)
        hipLaunchKernelGGL(layernorm_backward_kernel<true>, grid, dim3(256), 0, s, x, dy, g, rows, W, out);
    else
        hipLaunchKernelGGL(layernorm_backward_kernel<false>, grid, dim3(256), 0, s, x, dy, g, rows, W, out);
    LAUNCH_CHECK();
    return MPREID_OK;
}

int launch_quickgelu_backward(const float *u, float *d, int64_t n4, hipStream_t s) {
    hipLaunchKernelGGL(quickgelu_backward_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, u, d, n4);
    LAUNCH_CHECK();
    return MPREID_OK;
}

namespace {

// The backward call's workspace: the forward's regions first (f.x doubles as the block mid-point and f.hbuf as the fp32 FC1
// pre-activation of the sweep: the same 16 W bytes per row), then the kept block inputs and the gradient buffers
struct TextGradLayout {
    TextLayout f;
    SweepRegions r;
    size_t total;
};

TextGradLayout text_grad_layout(const mpreid_text_cfg *c, int B) {
    TextGradLayout v{};
    v.f = text_layout(c, B);
    WsCursor take{v.f.total};
    v.r = take_sweep_regions(take, (size_t)v.f.Mpad * c->width * 4, c->layers);
    v.total = take.off;
    return v;
}

}   // namespace

extern "C" size_t mpreid_text_backward_workspace_bytes(const mpreid_text_cfg *cfg, int batch) {
    if (!cfg || batch <= 0 || cfg->tokens <= 0 || cfg->width <= 0 || cfg->layers < 0) return 0;
    return text_grad_layout(cfg, batch).total;
}

extern "C" int mpreid_text_attention_backward(const float *qkv, const float *d_o, int B, int L, int W, int heads, float *d_qkv,
                                              mpreid_stream_t stream) {
    ARG_CHECK(qkv && d_o && d_qkv && B > 0);
    ARG_CHECK(((uintptr_t)qkv & 15) == 0 && ((uintptr_t)d_o & 15) == 0 && ((uintptr_t)d_qkv & 15) == 0);
    const int rc = text_check_shape(L, W, heads);
    if (rc) return rc;
    ARG_CHECK((int64_t)B * heads < (int64_t)1 << 31 && (int64_t)B * L * 3 * W < (int64_t)1 << 40);
    return launch_causal_attention_backward(qkv, d_o, B, L, W, heads, d_qkv, (hipStream_t)stream);
}

extern "C" int mpreid_layernorm_backward_f32(const float *x, const float *dy, const float *gamma, int64_t rows, int width,
                                             int accumulate, float *dx, mpreid_stream_t stream) {
    ARG_CHECK(x && dy && gamma && dx && rows >= 0 && width > 0);
    ARG_CHECK(rows < (int64_t)1 << 33);
    if (rows == 0) return MPREID_OK;
    return launch_layernorm_backward(x, dy, gamma, rows, width, accumulate != 0, dx, (hipStream_t)stream);
}

extern "C" int mpreid_quickgelu_backward_f32(const float *u, float *d, int64_t n, mpreid_stream_t stream) {
    ARG_CHECK(u && d && n >= 0 && n % 4 == 0);
    ARG_CHECK((((uintptr_t)u | (uintptr_t)d) & 15) == 0);
    ARG_CHECK(n < (int64_t)1 << 40);
    if (n == 0) return MPREID_OK;
    return launch_quickgelu_backward(u, d, n / 4, (hipStream_t)stream);
}

extern "C" int mpreid_text_backward(const mpreid_text_cfg *cfg, const mpreid_text_weights *w, const mpreid_text_weights_t *wt,
                                    const float *prompts, const int32_t *eot, const float *grad_out, int B, float *grad_prompts,
                                    void *ws, size_t ws_bytes, mpreid_stream_t stream_) {
    int rc = text_check_cfg(cfg);
    if (rc) return rc;
    ARG_CHECK(w && wt && prompts && eot && grad_out && grad_prompts && B > 0);
    ARG_CHECK(w->pos_emb && w->ln_final_g && w->ln_final_b && w->proj && wt->proj_t && ((w->layers && wt->layers) || cfg->layers == 0));
    ARG_CHECK(((uintptr_t)prompts & 15) == 0 && ((uintptr_t)w->pos_emb & 15) == 0 && ((uintptr_t)eot & 3) == 0 &&
              ((uintptr_t)grad_out & 3) == 0 && ((uintptr_t)grad_prompts & 15) == 0 && ((uintptr_t)wt->proj_t & 3) == 0);
    ARG_CHECK((int64_t)B * cfg->tokens <= ((int64_t)1 << 31) - 256);   // GemmArgs::M is an int
    for (int l = 0; l < cfg->layers; ++l) {
        const mpreid_text_layer_t &t = wt->layers[l];
        ARG_CHECK(t.in_proj_t && t.out_proj_t && t.fc_t && t.proj_t);
        ARG_CHECK((((uintptr_t)t.in_proj_t | (uintptr_t)t.out_proj_t | (uintptr_t)t.fc_t | (uintptr_t)t.proj_t) & 15) == 0);
    }
    const TextGradLayout v = text_grad_layout(cfg, B);
    if (!ws || ws_bytes < v.total) {
        mpreid_set_error("text backward workspace too small: %zu < %zu", ws_bytes, v.total);
        return MPREID_ERR_WORKSPACE;
    }
    ARG_CHECK(((uintptr_t)ws & 255) == 0);
    hipStream_t stream = (hipStream_t)stream_;
    const int W = cfg->width, L = cfg->tokens, M = (int)v.f.M, Mpad = (int)v.f.Mpad;
    char *base = (char *)ws;
    auto f32 = [&](size_t off) { return (float *)(base + off); };
    _Float16 *hbuf = (_Float16 *)(base + v.f.hbuf);
    // no parameter gradient: aot, at, bt, stats and red stay NULL and the workspace has no such regions.  u is the sweep's use
    // of the hbuf region
    BlockGrad c{};
    c.s = {W, cfg->heads, B, L, true}; c.Mpad = Mpad; c.stream = stream;
    c.x = f32(v.f.x); c.a = (_Float16 *)(base + v.f.a); c.qkv = f32(v.f.qkv); c.u = f32(v.f.hbuf);
    c.dx = f32(v.r.dx); c.dh = f32(v.r.dh); c.t = f32(v.r.t); c.dqkv = f32(v.r.dqkv);
    float *xs = f32(v.r.xs);
    const size_t xbytes = (size_t)M * W * 4, xstride = (size_t)Mpad * W;
    const mpreid_vit_layer_grads none{};

    // the forward, keeping x_l
    if ((rc = text_embed(prompts, w->pos_emb, v.f.M, L, W, c.x, stream))) return rc;
    for (int l = 0; l < cfg->layers; ++l) {
        HIP_TRY(hipMemcpyAsync(xs + l * xstride, c.x, xbytes, hipMemcpyDeviceToDevice, stream));
        if ((rc = tower_block(c.s, w->layers[l], c.x, c.a, c.qkv, hbuf, Mpad, stream))) return rc;
    }
    // text_projection and ln_final at the read-out rows -> d/dx_layers; zero everywhere else
    hipLaunchKernelGGL(text_head_backward_kernel, dim3((unsigned)B), dim3(256), 0, stream, c.x, eot, grad_out, L, W, cfg->out_dim,
                       wt->proj_t, w->ln_final_g, c.dx);
    LAUNCH_CHECK();
    for (int l = cfg->layers - 1; l >= 0; --l) {
        const float *xl = xs + l * xstride;
        HIP_TRY(hipMemcpyAsync(c.x, xl, xbytes, hipMemcpyDeviceToDevice, stream));
        if ((rc = tower_block_attention(c.s, w->layers[l], c.x, c.a, c.qkv, Mpad, stream))) return rc;
        if ((rc = block_mlp_backward(c, w->layers[l], wt->layers[l], none))) return rc;
        if ((rc = block_attention_backward(c, w->layers[l], wt->layers[l], xl, none))) return rc;   // dx = d/dx_l
    }
    // the positional embedding is an added constant: d/dprompts = d/dx_0
    HIP_TRY(hipMemcpyAsync(grad_prompts, c.dx, xbytes, hipMemcpyDeviceToDevice, stream));
    return MPREID_OK;
}
