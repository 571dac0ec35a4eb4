// optim.hip — stage-2 training around the image tower (include/mpreid.h): one optimizer step over a TABLE of tensors and the
// largest finite |entry| of a table of tensors.  Both take their table on the host, cut every tensor into work chunks of
// MPREID_OPTIM_CHUNK elements and hand the chunks of up to OPT_MAX_T tensors to one launch, the tensors' descriptors passed BY VALUE
// in the kernel arguments: nothing is uploaded, nothing is synchronised, no atomics.  The kernels are memory-bound (Adam: 4 reads
// and 3 writes of 4 bytes per element): 16-byte accesses where an entry's buffers allow them, a grid capped at OPT_MAX_GRID
// workgroups of 256 that stride over the chunks, so a 2.4 M-element matrix and a 768-element bias of one launch share the chip.
// Strict IEEE arithmetic (the plain flag set, as prompt_train.hip): the bits of an update are defined.
#include "common.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr int OPT_CHUNK = MPREID_OPTIM_CHUNK;   // elements per work chunk: a multiple of 4, so a chunk keeps its tensor's alignment
constexpr int OPT_MAX_T = MPREID_OPTIM_TENSORS_PER_LAUNCH;
constexpr int OPT_MAX_GRID = 2048;
constexpr int64_t OPT_MAX_N = (int64_t)1 << 38;          // elements of one tensor
constexpr int64_t OPT_MAX_CHUNKS = (int64_t)1 << 30;     // chunks of one launch (an int)
static_assert(OPT_CHUNK % 4 == 0 && OPT_CHUNK >= 1024, "a chunk is whole float4 groups, four per thread or more");

// what every kernel here does first: the chunk -> tensor map of its launch into LDS (first[t] = the launch's first chunk of
// tensor t, ascending; first[n_t] = the number of chunks), and then per chunk the tensor that holds it, the same in every lane
template <typename Launch>
__device__ __forceinline__ void load_chunk_map(const Launch &L, int *first) {
    for (int t = threadIdx.x; t <= L.n_t; t += 256) first[t] = t < L.n_t ? L.t[t].first_chunk : L.chunks;
    __syncthreads();
}

__device__ __forceinline__ int tensor_of_chunk(const int *first, int n_t, int c) {
    int lo = 0, hi = n_t - 1;   // the largest t with first[t] <= c
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (first[mid] <= c)
            lo = mid;
        else
            hi = mid - 1;
    }
    return __builtin_amdgcn_readfirstlane(lo);
}

// ---------------------------------------------------------------------------------------------------------------------
// the optimizer step
// ---------------------------------------------------------------------------------------------------------------------
struct OptTensor {
    float *p;
    const float *g;
    float *s1, *s2;
    int64_t n;
    int first_chunk;
    int cls_vec;   // hyper-parameter class | (all four buffers 16-byte aligned) << 8
};

struct OptClass {
    float a, wd, lw;   // Adam / AdamW: a = lr / (1 - beta1^step), lw = lr * wd.  SGD: a = lr
};

struct OptLaunch {
    OptTensor t[OPT_MAX_T];
    OptClass c[MPREID_OPTIM_MAX_CLASSES];
    float w1, beta2, w2, r, eps, mu;
    int n_t, chunks, first_step;
};
static_assert(sizeof(OptLaunch) <= 4096, "the launch descriptor travels in the kernel arguments");

struct OptArgs {   // one class's constants beside the launch's
    float w1, beta2, w2, a, r, eps, wd, lw, mu;
    int first_step;
};

// the lines of adam_one (prompt_train.hip, include/mpreid.h "mpreid_adam_step_f32"), unchanged: the same bits
template <int ALGO>
__device__ __forceinline__ void optim_one(float &p, float g, float &m, float &v, const OptArgs &c) {
    if (ALGO == MPREID_OPTIM_SGD) {
        g = fmaf(c.wd, p, g);
        m = c.first_step ? g : fmaf(c.mu, m, g);
        p = fmaf(-c.a, m, p);
        return;
    }
    if (ALGO == MPREID_OPTIM_ADAMW)
        p = fmaf(-c.lw, p, p);
    else
        g = fmaf(c.wd, p, g);
    m = fmaf(c.w1, g - m, m);
    v = fmaf(c.w2, g * g, c.beta2 * v);
    p = fmaf(-c.a, __fdiv_rn(m, __fdiv_rn(sqrtf(v), c.r) + c.eps), p);
}

template <int ALGO>
__global__ __launch_bounds__(256) void optim_multi_kernel(const OptLaunch L) {
    __shared__ int first[OPT_MAX_T + 1];
    load_chunk_map(L, first);
    constexpr bool ADAM = ALGO != MPREID_OPTIM_SGD;
    for (int chunk = blockIdx.x; chunk < L.chunks; chunk += gridDim.x) {
        const OptTensor &e = L.t[tensor_of_chunk(first, L.n_t, chunk)];
        const OptClass &k = L.c[e.cls_vec & 255];
        const OptArgs c{L.w1, L.beta2, L.w2, k.a, L.r, L.eps, k.wd, k.lw, L.mu, L.first_step};
        const int64_t off = (int64_t)(chunk - e.first_chunk) * OPT_CHUNK;
        const int cnt = (int)min((int64_t)OPT_CHUNK, e.n - off);
        float *p = e.p + off, *m = e.s1 + off, *v = ADAM ? e.s2 + off : nullptr;
        const float *g = e.g + off;
        const int n4 = (e.cls_vec >> 8) ? cnt / 4 : 0;   // groups of four through 16-byte accesses, the rest one by one
        for (int i = threadIdx.x; i < n4; i += 256) {
            float4 pp = reinterpret_cast<float4 *>(p)[i], mm = reinterpret_cast<float4 *>(m)[i];
            float4 vv = ADAM ? reinterpret_cast<float4 *>(v)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
            const float4 gg = reinterpret_cast<const float4 *>(g)[i];
            optim_one<ALGO>(pp.x, gg.x, mm.x, vv.x, c);
            optim_one<ALGO>(pp.y, gg.y, mm.y, vv.y, c);
            optim_one<ALGO>(pp.z, gg.z, mm.z, vv.z, c);
            optim_one<ALGO>(pp.w, gg.w, mm.w, vv.w, c);
            reinterpret_cast<float4 *>(p)[i] = pp;
            reinterpret_cast<float4 *>(m)[i] = mm;
            if (ADAM) reinterpret_cast<float4 *>(v)[i] = vv;
        }
        for (int i = 4 * n4 + threadIdx.x; i < cnt; i += 256) {
            float vv = ADAM ? v[i] : 0.f;
            optim_one<ALGO>(p[i], g[i], m[i], vv, c);
            if (ADAM) v[i] = vv;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// the largest finite |entry| per tensor: a partial per chunk, then one workgroup per tensor over its partials
// ---------------------------------------------------------------------------------------------------------------------
struct MaxTensor {
    const float *src;
    int64_t n;
    int first_chunk;
    int vec;
};

struct MaxLaunch {
    MaxTensor t[OPT_MAX_T];
    float *partial;   // [chunks] of this launch
    float *out;       // [n_t] of this launch
    int n_t, chunks;
};
static_assert(sizeof(MaxLaunch) <= 4096, "the launch descriptor travels in the kernel arguments");

__device__ __forceinline__ float finite_abs(float x) {
    x = fabsf(x);
    return x < INFINITY ? x : 0.f;   // NaN and the infinities count as 0
}

// the maximum over a workgroup's 256 values, valid in thread 0 (all values are >= 0 and finite)
__device__ __forceinline__ float block_max(float s, float *red) {
    s = wave_bfly_max(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    const float r = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(256) void absmax_chunks_kernel(const MaxLaunch L) {
    __shared__ int first[OPT_MAX_T + 1];
    __shared__ float red[4];
    load_chunk_map(L, first);
    for (int chunk = blockIdx.x; chunk < L.chunks; chunk += gridDim.x) {
        const MaxTensor &e = L.t[tensor_of_chunk(first, L.n_t, chunk)];
        const int64_t off = (int64_t)(chunk - e.first_chunk) * OPT_CHUNK;
        const int cnt = (int)min((int64_t)OPT_CHUNK, e.n - off);
        const float *x = e.src + off;
        const int n4 = e.vec ? cnt / 4 : 0;
        float s = 0.f;
        for (int i = threadIdx.x; i < n4; i += 256) {
            const float4 q = reinterpret_cast<const float4 *>(x)[i];
            s = fmaxf(fmaxf(s, fmaxf(finite_abs(q.x), finite_abs(q.y))), fmaxf(finite_abs(q.z), finite_abs(q.w)));
        }
        for (int i = 4 * n4 + threadIdx.x; i < cnt; i += 256) s = fmaxf(s, finite_abs(x[i]));
        s = block_max(s, red);
        if (threadIdx.x == 0) L.partial[chunk] = s;
    }
}

__global__ __launch_bounds__(256) void absmax_final_kernel(const MaxLaunch L) {
    __shared__ float red[4];
    const int t = blockIdx.x;   // < n_t
    const int c0 = L.t[t].first_chunk, c1 = t + 1 < L.n_t ? L.t[t + 1].first_chunk : L.chunks;
    float s = 0.f;
    for (int c = c0 + threadIdx.x; c < c1; c += 256) s = fmaxf(s, L.partial[c]);
    s = block_max(s, red);
    if (threadIdx.x == 0) L.out[t] = s;
}

int64_t chunks_of(int64_t n) { return (n + OPT_CHUNK - 1) / OPT_CHUNK; }

int check_absmax_table(const mpreid_absmax_entry *entries, int n_entries) {
    ARG_CHECK(entries && n_entries >= 1);
    for (int i = 0; i < n_entries; ++i) {
        if (!entries[i].src_dev || ((uintptr_t)entries[i].src_dev & 3) || entries[i].n < 1 || entries[i].n >= OPT_MAX_N) {
            mpreid_set_error("bad argument: absmax table entry %d (a NULL or misaligned pointer, or n = %lld outside 1 .. 2^38 - 1)", i,
                             (long long)entries[i].n);
            return MPREID_ERR_ARG;
        }
    }
    return MPREID_OK;
}

}   // namespace

extern "C" int mpreid_optim_step_launches(int n_entries) {
    return n_entries < 1 ? 0 : (n_entries + OPT_MAX_T - 1) / OPT_MAX_T;
}

extern "C" int mpreid_optim_step_multi_f32(const mpreid_optim_entry *entries, int n_entries, const mpreid_optim_class *classes,
                                           int n_classes, int algo, int step, float beta1, float beta2, float eps, float momentum,
                                           mpreid_stream_t stream) {
    ARG_CHECK(entries && n_entries >= 1 && classes && n_classes >= 1 && n_classes <= MPREID_OPTIM_MAX_CLASSES);
    ARG_CHECK(algo == MPREID_OPTIM_SGD || algo == MPREID_OPTIM_ADAM || algo == MPREID_OPTIM_ADAMW);
    ARG_CHECK(step >= 1);
    const bool adam = algo != MPREID_OPTIM_SGD;
    if (adam)
        ARG_CHECK(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f && std::isfinite(eps) && eps > 0.f);
    else
        ARG_CHECK(std::isfinite(momentum) && momentum >= 0.f);
    for (int k = 0; k < n_classes; ++k) {
        const float lr = classes[k].lr, wd = classes[k].weight_decay;
        if (!(std::isfinite(lr) && lr >= 0.f && std::isfinite(wd) && wd >= 0.f)) {
            mpreid_set_error("bad argument: optimizer class %d: lr and weight_decay must be finite and >= 0", k);
            return MPREID_ERR_ARG;
        }
    }
    for (int i = 0; i < n_entries; ++i) {
        const mpreid_optim_entry &e = entries[i];
        const uintptr_t all = (uintptr_t)e.param_dev | (uintptr_t)e.grad_dev | (uintptr_t)e.state1_dev | (uintptr_t)(adam ? e.state2_dev : nullptr);
        if (!e.param_dev || !e.grad_dev || !e.state1_dev || (adam && !e.state2_dev) || (all & 3) || e.n < 1 || e.n >= OPT_MAX_N ||
            e.hyper < 0 || e.hyper >= n_classes) {
            mpreid_set_error("bad argument: optimizer table entry %d (a NULL or misaligned pointer, n = %lld outside 1 .. 2^38 - 1, or "
                             "class %d outside 0 .. %d)", i, (long long)e.n, (int)e.hyper, n_classes - 1);
            return MPREID_ERR_ARG;
        }
    }
    OptLaunch L{};
    L.w1 = (float)(1.0 - (double)beta1);
    L.beta2 = beta2;
    L.w2 = (float)(1.0 - (double)beta2);
    L.r = adam ? (float)std::sqrt(1.0 - std::pow((double)beta2, (double)step)) : 1.f;
    L.eps = eps;
    L.mu = momentum;
    L.first_step = step == 1;
    for (int k = 0; k < n_classes; ++k) {
        const double lr = (double)classes[k].lr;
        L.c[k].a = adam ? (float)(lr / (1.0 - std::pow((double)beta1, (double)step))) : classes[k].lr;
        L.c[k].wd = classes[k].weight_decay;
        L.c[k].lw = (float)(lr * (double)classes[k].weight_decay);
    }
    for (int i0 = 0; i0 < n_entries;) {
        int64_t chunks = 0;
        int n_t = 0;
        while (i0 + n_t < n_entries && n_t < OPT_MAX_T && chunks + chunks_of(entries[i0 + n_t].n) <= OPT_MAX_CHUNKS) {
            const mpreid_optim_entry &e = entries[i0 + n_t];
            const uintptr_t all = (uintptr_t)e.param_dev | (uintptr_t)e.grad_dev | (uintptr_t)e.state1_dev | (uintptr_t)(adam ? e.state2_dev : nullptr);
            L.t[n_t] = OptTensor{e.param_dev, e.grad_dev, e.state1_dev, adam ? e.state2_dev : nullptr, e.n, (int)chunks,
                                 e.hyper | ((all & 15) == 0 ? 256 : 0)};
            chunks += chunks_of(e.n);
            ++n_t;
        }
        L.n_t = n_t;
        L.chunks = (int)chunks;
        const dim3 grid((unsigned)std::min<int64_t>(chunks, OPT_MAX_GRID));
        if (algo == MPREID_OPTIM_SGD)
            hipLaunchKernelGGL(optim_multi_kernel<MPREID_OPTIM_SGD>, grid, dim3(256), 0, (hipStream_t)stream, L);
        else if (algo == MPREID_OPTIM_ADAM)
            hipLaunchKernelGGL(optim_multi_kernel<MPREID_OPTIM_ADAM>, grid, dim3(256), 0, (hipStream_t)stream, L);
        else
            hipLaunchKernelGGL(optim_multi_kernel<MPREID_OPTIM_ADAMW>, grid, dim3(256), 0, (hipStream_t)stream, L);
        LAUNCH_CHECK();
        i0 += n_t;
    }
    return MPREID_OK;
}

extern "C" size_t mpreid_absmax_multi_workspace_bytes(const mpreid_absmax_entry *entries, int n_entries) {
    if (check_absmax_table(entries, n_entries) != MPREID_OK) return 0;
    int64_t chunks = 0;
    for (int i = 0; i < n_entries; ++i) chunks += chunks_of(entries[i].n);
    return align_up((size_t)chunks * sizeof(float), 256);
}

extern "C" int mpreid_absmax_multi_f32(const mpreid_absmax_entry *entries, int n_entries, float *out_dev, void *ws_dev,
                                       size_t ws_bytes, mpreid_stream_t stream) {
    const int rc = check_absmax_table(entries, n_entries);
    if (rc != MPREID_OK) return rc;
    ARG_CHECK(out_dev && ((uintptr_t)out_dev & 3) == 0);
    const size_t need = mpreid_absmax_multi_workspace_bytes(entries, n_entries);
    if (!ws_dev || ws_bytes < need) {
        mpreid_set_error("absmax workspace too small: %zu < %zu", ws_bytes, need);
        return MPREID_ERR_WORKSPACE;
    }
    ARG_CHECK(((uintptr_t)ws_dev & 255) == 0);
    float *partial = (float *)ws_dev;
    MaxLaunch L{};
    for (int i0 = 0; i0 < n_entries;) {
        int64_t chunks = 0;
        int n_t = 0;
        while (i0 + n_t < n_entries && n_t < OPT_MAX_T && chunks + chunks_of(entries[i0 + n_t].n) <= OPT_MAX_CHUNKS) {
            const mpreid_absmax_entry &e = entries[i0 + n_t];
            L.t[n_t] = MaxTensor{e.src_dev, e.n, (int)chunks, ((uintptr_t)e.src_dev & 15) == 0};
            chunks += chunks_of(e.n);
            ++n_t;
        }
        L.n_t = n_t;
        L.chunks = (int)chunks;
        L.partial = partial;
        L.out = out_dev + i0;
        hipLaunchKernelGGL(absmax_chunks_kernel, dim3((unsigned)std::min<int64_t>(chunks, OPT_MAX_GRID)), dim3(256), 0,
                           (hipStream_t)stream, L);
        LAUNCH_CHECK();
        hipLaunchKernelGGL(absmax_final_kernel, dim3((unsigned)n_t), dim3(256), 0, (hipStream_t)stream, L);
        LAUNCH_CHECK();
        partial += chunks;
        i0 += n_t;
    }
    return MPREID_OK;
}
