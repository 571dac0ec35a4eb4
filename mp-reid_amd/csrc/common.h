// common.h — shared host/device helpers of libmpreid_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <mutex>

#include "../../include/mpreid.h"
#include "../../include/mpreid_numerics.h"

void mpreid_set_error(const char *fmt, ...);

#define HIP_TRY(expr)                                                                               \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess) {                                                                     \
            mpreid_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return (int)e_;                                                                         \
        }                                                                                           \
    } while (0)
#define LAUNCH_CHECK() HIP_TRY(hipGetLastError())
#define ARG_CHECK(cond)                                                                             \
    do {                                                                                            \
        if (!(cond)) {                                                                              \
            mpreid_set_error("bad argument: %s (%s:%d)", #cond, __FILE__, __LINE__);               \
            return MPREID_ERR_ARG;                                                                  \
        }                                                                                           \
    } while (0)

// The one check of a caller's image batch (include/mpreid.h: mpreid_image_in), run by every encoder forward before its
// first HIP runtime call.  *in receives what the kernels take BY VALUE: the caller's struct, with mean 0 / std 1 in place
// of whatever an fp32 batch left there (those fields are read only with uint8 input).
static inline int mpreid_check_image_in(const mpreid_image_in *img, mpreid_image_in *in) {
    if (!img) {
        mpreid_set_error("bad argument: the image descriptor (mpreid_image_in) is NULL");
        return MPREID_ERR_ARG;
    }
    if ((img->f32_dev != nullptr) == (img->u8_hwc_dev != nullptr)) {
        mpreid_set_error("bad argument: mpreid_image_in needs exactly one of f32_dev and u8_hwc_dev (%s are set)",
                         img->f32_dev ? "both" : "neither");
        return MPREID_ERR_ARG;
    }
    if (img->view < MPREID_VIEW_ORIGINAL || img->view > MPREID_VIEW_PSEUDO_RGB) {
        mpreid_set_error("bad argument: mpreid_image_in.view = %d is none of MPREID_VIEW_* (0..3)", (int)img->view);
        return MPREID_ERR_ARG;
    }
    *in = *img;
    if (img->f32_dev)
        for (int c = 0; c < 3; ++c) {
            in->mean[c] = 0.f;
            in->std[c] = 1.f;
        }
    return MPREID_OK;
}

__host__ __device__ static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// the 256-byte aligned bump cursor of every workspace layout (towers, re-ranking): take(bytes) -> offset
struct WsCursor {
    size_t off = 0;
    size_t operator()(size_t bytes) { const size_t o = off; off += align_up(bytes, 256); return o; }
};

// Timing-ablation switches (MPREID_GEMM_DBG, MPREID_ATT_DBG, MPREID_CAND_DBG, MPREID_JACCARD_DBG: kernels that skip loads,
// matrix instructions or stores -- WRONG RESULTS by design) are honoured only by a library built with -DMPREID_ABLATION
// (MPREID_ABLATION=1 python mp-reid_amd/mpreid/build.py); the shipped library ignores them, so a stray environment
// variable cannot change results.  The GEMM kernels' ablation INSTANCES (template arguments, the lists in
// gemm_plan.h) are named inside #ifdef MPREID_ABLATION only, so the shipped library does not even contain them.
static inline int mpreid_ablation_env(const char *name) {
#ifdef MPREID_ABLATION
    const char *e = getenv(name);
    return e ? atoi(e) : 0;
#else
    (void)name;
    return 0;
#endif
}

// Tuning switches between BIT-IDENTICAL forms of a stage (kernel shape selection, side-stream overlap): ONE documented
// environment string, MPREID_TUNE="key=value,key=value" (include/mpreid.h lists the keys), read once per process.  A key that
// is absent returns `dflt`; unknown keys are reported once on stderr -- a stray or misspelt variable cannot silently change
// which kernel is measured.  (Switches that change RESULTS exist only in -DMPREID_ABLATION builds, above.)
int mpreid_tune(const char *key, int dflt);

// Bijective XCD-aware remap of a 1-D block id: blocks b and b+8 share an XCD (round-robin
// dispatch), so give each XCD a contiguous chunk of the logical tile order (L2 locality only;
// correctness never depends on it).  cdna_hip_programming.md §5 "XCD swizzle must be bijective".
__device__ __forceinline__ unsigned xcd_remap(unsigned orig, unsigned nwg) {
    const unsigned q = nwg >> 3, r = nwg & 7u, xcd = orig & 7u;
    const unsigned base = (xcd < r) ? xcd * (q + 1u) : r * (q + 1u) + (xcd - r) * q;
    return base + (orig >> 3);
}

// grouped tile order: walk GM tile-rows at a time so concurrently resident blocks share B panels
__device__ __forceinline__ void tile_coords(unsigned id, int tiles_m, int tiles_n, int GM, int &tm, int &tn) {
    const unsigned per_group = (unsigned)GM * (unsigned)tiles_n;
    const unsigned group = id / per_group;
    const int first_m = (int)group * GM;
    const int gsize = min(tiles_m - first_m, GM);
    const unsigned in_group = id % per_group;
    tm = first_m + (int)(in_group % (unsigned)gsize);
    tn = (int)(in_group / (unsigned)gsize);
}

// fp16 PAIR split of the `split` precision modes, x = hi + lo with hi = fp16(x), lo = fp16(x - float(hi)), two values at a
// time in THREE instructions: v_cvt_pk_f16_f32 (both hi), then v_fma_mixlo_f16 / v_fma_mixhi_f16 computing fma(hi, -1, x)
// from the packed hi halves and rounding it once into the low / high half of the packed lo.  x - hi is exact in fp32, so the
// single rounding gives the bits of the plain form (tools/probes/mix_probe.hip: 2^25 pairs incl. 14 M subnormal lo, 0
// mismatches); hipcc compiles the plain form to 6.5 instructions per two values (separate conversions back to fp32, subtract,
// convert, pack) and folds fma(hi, -1, x) back into a subtraction, hence the inline assembly.
typedef _Float16 mp_h2_t __attribute__((ext_vector_type(2)));
typedef float mp_f2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void split_pair2(float x0, float x1, mp_h2_t &hi, mp_h2_t &lo) {
    hi = __builtin_convertvector(mp_f2_t{x0, x1}, mp_h2_t);
    const unsigned hb = __builtin_bit_cast(unsigned, hi);
    unsigned d;
    asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(d) : "v"(hb), "v"(x0));
    asm("v_fma_mixhi_f16 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(d) : "v"(hb), "v"(x1));
    lo = __builtin_bit_cast(mp_h2_t, d);
}
// N values (N even) -> vectors of N halves (any ext_vector_type of _Float16 with N elements)
template <int N, typename HV>
__device__ __forceinline__ void split_pairs(const float (&x)[N], HV &hi, HV &lo) {
    static_assert(N % 2 == 0, "pairs");
#pragma unroll
    for (int j = 0; j < N; j += 2) {
        mp_h2_t h, l;
        split_pair2(x[j], x[j + 1], h, l);
        hi[j] = h[0]; hi[j + 1] = h[1];
        lo[j] = l[0]; lo[j + 1] = l[1];
    }
}

// The ranking key of a matrix entry (evalrank.hip, ranklist.hip): ascending as an unsigned 64-bit integer = ascending
// (distance, idx) with -0 equal to +0 -- the order a stable argsort of a NaN-free row gives.
__device__ __forceinline__ unsigned long long ev_key(float f, unsigned idx) {
    f = f + 0.0f; // -0 -> +0
    unsigned u = __float_as_uint(f);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)u << 32) | idx;
}

__device__ __forceinline__ float wave_bfly_add(float s) {
    // fixed butterfly 32,16,8,4,2,1 — the order the oracle mirrors (oracle/mpreid_oracle.c sqnorm_row)
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s = s + __shfl_xor(s, off, 64);
    return s;
}

__device__ __forceinline__ float wave_bfly_max(float s) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s = fmaxf(s, __shfl_xor(s, off, 64));
    return s;
}

// LDS written by this wave is read by this wave
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// sum_c a[c] * b[c] over the 64 features of a head, c ascending in one fmaf chain: the SAME bits wherever a score is needed
__device__ __forceinline__ float dot64(const float *__restrict__ a, const float *__restrict__ b) {
    float acc = 0.f;
#pragma unroll
    for (int c = 0; c < 64; c += 4) {
        const float4 x = *reinterpret_cast<const float4 *>(a + c);
        const float4 y = *reinterpret_cast<const float4 *>(b + c);
        acc = fmaf(x.x, y.x, acc);
        acc = fmaf(x.y, y.y, acc);
        acc = fmaf(x.z, y.z, acc);
        acc = fmaf(x.w, y.w, acc);
    }
    return acc;
}

// Per-launch event timing shared by the kernels bench.py reports a roofline for (gemm_f16.hip owns the registry).
// prof_begin returns an opaque token (nullptr while profiling is disabled); prof_end records the closing event and files
// the launch under (cls, m, n, k) with `work` = executed FLOPs (matrix kernels) or algorithmic bytes (HBM-bound kernels).
// cls: a GemmEpi id for the fp16 GEMM kernels, MPREID_PROF_* for the others.
void *mpreid_prof_begin(hipStream_t stream);
bool mpreid_prof_active(); // mpreid_profile_enable(1) is in force: a launcher whose work figure costs something computes it only then
void mpreid_prof_end(void *token, hipStream_t stream, int cls, int64_t m, int n, int k, double work);

// The ONE way a launcher asks for `bytes` of dynamic LDS for `kernel`, called before every launch that passes them:
// MPREID_ERR_UNSUPPORTED above 160 KiB (one workgroup's LDS on gfx950), nothing to do up to 48 KiB (what a launch may pass
// without the attribute), and in between hipFuncAttributeMaxDynamicSharedMemorySize is raised when `bytes` exceeds what
// this kernel was last given on the CURRENT HIP device -- the attribute is per device and one process may drive several
// GPUs.  Grow-only, one table and one mutex (api.cpp); devices numbered 64 or higher are not cached, as in PerDeviceOnce.
// Returns MPREID_OK, or an mpreid / hip status with the error text set.
int mpreid_dyn_lds(const void *kernel, size_t bytes);
template <typename F>
static inline int mpreid_dyn_lds(F *kernel, size_t bytes) {
    return mpreid_dyn_lds(reinterpret_cast<const void *>(kernel), bytes);
}

// CU count of the CURRENT HIP device, for the launchers that size a persistent grid by it: asked of the runtime once per
// device and cached (api.cpp); devices numbered 64 or higher are not cached, as in PerDeviceOnce.
int mpreid_device_cus(int *cus);

// Run `f` (returns an mpreid/hip status) once per HIP device for the call site that owns this object: whatever else is
// per device (occupancy queries, a verbose line) -- one process may drive several GPUs.  The dynamic-LDS attribute has
// its own rule: mpreid_dyn_lds above.
struct PerDeviceOnce {
    std::mutex mu;
    bool done[64] = {};
    template <typename F>
    int run(F f) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) dev = 0;
        std::lock_guard<std::mutex> lk(mu);
        if (dev >= 0 && dev < 64 && done[dev]) return MPREID_OK;
        const int rc = f();
        if (rc == MPREID_OK && dev >= 0 && dev < 64) done[dev] = true;
        return rc;
    }
};
