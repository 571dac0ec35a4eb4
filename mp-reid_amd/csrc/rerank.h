// rerank.h — what the re-ranking files share (k-reciprocal re-ranking on gfx950; reference: utils/reranking.py:29-100).
// rerank.hip (stages 7-11, the tail and the dense driver, the single-call and the row-sharded entry points),
// rerank_neighbours.hip (stages 1-6), rerank_sparse.hip (candidate pipeline), rerank_wide.hip (any k): DESIGN.md has the map.  A kernel lives in the file of the launcher that launches it; what a second file needs is declared here.
//
// Data layout in HBM (all inside the caller's workspace, see make_layout()):
//   feat  [N][d] fp32          cat(probFea, galFea)                                  (:36)
//   D     [N][ld] fp32         all-pairs squared distance, exact fp32 MFMA GEMM      (:36-41)
//                              ld = N rounded up to 64 floats; D is bit-symmetric
//   MT    [N][ld] fp32         only with local_distmat: (D + local)^T                (:43-46)
//   rowmax[N]                  max over column i of original_dist == row max of MT   (:46)
//   rank  [N][KR] int32        first KR = max(k1+1, k2) entries of argsort(O[i,:])   (:48)
//                              O[i][j] = MT[i][j] / rowmax[i] is recomputed where needed
//   V     ELL  idx[N][vcap] int32 ascending, val[N][vcap] fp16 bits, cnt[N]           (:51-71)
//   Vqe   ELL  same, row stride = measured max union size                             (:73-78)
//   CSC of Vqe: cptr[N+1] int64, crow[nnz] int32, cval[nnz] fp16 bits                  (:80-82)
//   out   [nq][ldo] fp32       final_dist[:nq, nq:]                                   (:84-100)
//
// Every rounding point of SURVEY.md §8a row a7 is taken through include/mpreid_numerics.h, the
// same code the CPU oracle runs, so the result is bit-identical to oracle/mpreid_oracle.c.
// All kernels of these files are HBM/L2-bound integer+fp16 work (no MFMA); the GEMM is in distance.hip.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <functional>
#include <mutex>
#include <vector>

#include "common.h"
#include "gemm_f16.h"

int mpreid_distance_launch(const float *q, const float *g, int64_t nq, int64_t ng, int d, const float *qn,
                           const float *gn, float *out, int64_t ldo, int epi, hipStream_t stream,
                           const unsigned *m_count = nullptr);
// gemm_f16.hip: 3-term fp16-split distances (|error| <= 1e-6 on unit-norm rows)
int mpreid_distance_f16_split3(const float *q, const float *g, int64_t nq, int64_t ng, int d, const float *qn,
                               const float *gn, float *out, int64_t ldo, int epi, void *ws, size_t ws_bytes,
                               hipStream_t stream);
size_t mpreid_distance_split3_ws_bytes(int64_t nq, int64_t ng, int d);

// ---------------------------------------------------------------------------------------------
// Native binary16 on the device.  include/mpreid_numerics.h spells numpy's float16 arithmetic out in integer code
// (fp32 operation, then a branchy RNE conversion: ~50 instructions), which is what the oracle compiles.  On gfx950
// v_cvt_f16_f32 / v_cvt_f32_f16 / v_add_f16 are IEEE round-to-nearest-even with subnormals (the f16 denormal
// mode is always on), and "add in fp32, round to fp16" equals one correctly rounded fp16 add (double rounding is
// innocuous when the wide format has >= 2p+2 = 24 significand bits).  Same bits, one instruction: the Jaccard
// accumulation was ALU-bound on the integer form.  tests/test_gpu_rerank.py compares every output bit with the
// oracle, so a device on which this did not hold would fail there.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint16_t h_from_f32(float f) { return __builtin_bit_cast(uint16_t, (_Float16)f); }
__device__ __forceinline__ float h_to_f32(uint16_t h) { return (float)__builtin_bit_cast(_Float16, h); }
// numpy's float16 sub / mul / div, literally: the operation in fp32, one RNE conversion to fp16
__device__ __forceinline__ uint16_t h_sub_native(uint16_t a, uint16_t b) { return h_from_f32(h_to_f32(a) - h_to_f32(b)); }
__device__ __forceinline__ uint16_t h_mul_native(uint16_t a, uint16_t b) { return h_from_f32(h_to_f32(a) * h_to_f32(b)); }
__device__ __forceinline__ uint16_t h_div_native(uint16_t a, uint16_t b) {
    return h_from_f32(__fdiv_rn(h_to_f32(a), h_to_f32(b)));
}
__device__ __forceinline__ uint16_t h_add_native(uint16_t a, uint16_t b) {
    return __builtin_bit_cast(uint16_t, (_Float16)(__builtin_bit_cast(_Float16, a) + __builtin_bit_cast(_Float16, b)));
}

// ---------------------------------------------------------------------------------------------
// small device helpers
// ---------------------------------------------------------------------------------------------
// Inclusive scan over the 64 lanes with DPP moves (row_shr 1 / 2 / 4 / 8 inside the rows of 16 lanes, then row_bcast:15
// into rows 1 and 3 and row_bcast:31 into rows 2 and 3): six VALU operations.  The __shfl_up formulation compiles to
// ds_bpermute_b32 -- an LDS crossbar round trip per step, ~850 cycles per scan measured with in-kernel stamps: the ten
// scans of extract_bits_sorted were a third of a k-reciprocal row at N = 20 000, the 49 of the query expansion most of it
// at N = 100 000.
__device__ __forceinline__ int wave_incl_scan(int v) {
    int x = v;
    x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xf, 0xf, true);    // row_shr:1
    x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xf, 0xf, true);    // row_shr:2
    x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xf, 0xf, true);    // row_shr:4
    x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xf, 0xf, true);    // row_shr:8
    x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xa, 0xf, false);   // row_bcast:15 -> rows 1, 3
    x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xc, 0xf, false);   // row_bcast:31 -> rows 2, 3
    return x;
}
__device__ __forceinline__ int wave_excl_scan(int v, int lane, int &total) {
    (void)lane;
    const int x = wave_incl_scan(v);
    total = __builtin_amdgcn_readlane(x, 63);
    return x - v;
}

// orderable key of a float: ascending unsigned order == ascending float order (-0 folded into +0)
__device__ __forceinline__ uint32_t fkey(float f) {
    f = f + 0.0f;
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// numpy pairwise sum of a[0..n) (LDS or global), evaluated redundantly by every 8-lane group of
// the calling wave; all lanes return the same value.  Mirrors orc_pairwise_sum_f32.
__device__ float wave_pairwise_sum(const float *a, int n, int lane) {
    const int j = lane & 7;
    // explicit post-order traversal of the recursion  pw(o,n) = pw(o,n2) + pw(o+n2,n-n2)
    int st_off[24], st_n[24];
    float st_val[24];
    unsigned char st_state[24];
    int sp = 0;
    st_off[0] = 0; st_n[0] = n; st_state[0] = 0;
    float ret = 0.0f;
    while (sp >= 0) {
        const int o = st_off[sp], m = st_n[sp];
        if (st_state[sp] == 0) {
            if (m <= 128) {
                float res;
                if (m < 8) {
                    res = 0.0f;
                    for (int i = 0; i < m; ++i) res = res + a[o + i];
                } else {
                    float r = a[o + j];
                    const int lim = m - (m % 8);
                    int i;
                    for (i = 8; i < lim; i += 8) r = r + a[o + i + j];
                    r = r + __shfl_xor(r, 1, 64);
                    r = r + __shfl_xor(r, 2, 64);
                    r = r + __shfl_xor(r, 4, 64);
                    res = r;
                    for (i = lim; i < m; ++i) res = res + a[o + i];
                }
                ret = res;
                --sp;
            } else {
                int n2 = m / 2;
                n2 -= n2 % 8;
                st_state[sp] = 1;
                ++sp;
                st_off[sp] = o; st_n[sp] = n2; st_state[sp] = 0;
            }
        } else if (st_state[sp] == 1) {
            int n2 = m / 2;
            n2 -= n2 % 8;
            st_val[sp] = ret;
            st_state[sp] = 2;
            ++sp;
            st_off[sp] = o + n2; st_n[sp] = m - n2; st_state[sp] = 0;
        } else {
            ret = st_val[sp] + ret;
            --sp;
        }
    }
    return ret;
}

// exclusive scan over the 256 threads of a workgroup (s_wave: 4 ints of LDS); total = the sum over all of them
__device__ __forceinline__ int block_excl_scan_256(int v, int tid, int *s_wave, int &total) {
    const int lane = tid & 63, wave = tid >> 6;
    int wtot;
    const int ex = wave_excl_scan(v, lane, wtot);
    __syncthreads();
    if (lane == 0) s_wave[wave] = wtot;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const int t = s_wave[w];
        if (w < wave) base += t;
        tot += t;
    }
    total = tot;
    return base + ex;
}

// wpre (optional): wpre[w] = number of set bits below word w, written for the words of every non-empty group of 64 (the
// only ones a set bit can live in): slot(c) = wpre[c >> 5] + popc(mask[c >> 5] & below(c))
__device__ __forceinline__ int extract_bits_sorted(const unsigned *mask, int nw, int *list, int lane, int *wpre = nullptr) {
    int base = 0;
    for (int w0 = 0; w0 < nw; w0 += 64) {
        const int w = w0 + lane;
        unsigned word = (w < nw) ? mask[w] : 0u;
        if (__ballot(word != 0u) == 0ull) continue;
        int tot;
        int pos = base + wave_excl_scan(__popc(word), lane, tot);
        if (wpre && w < nw) wpre[w] = pos;
        while (word) {
            const int b = __ffs((int)word) - 1;
            word &= word - 1u;
            list[pos++] = w * 32 + b;
        }
        base += tot;
    }
    return base;
}

// exact squared distance of rows i and j of `feat`, the oracle's arithmetic (oracle/mpreid_oracle.c: dot_block +
// orc_euclid): a k-ascending fmaf chain from 0, then fmaf(-2, dot, |f_i|^2 + |f_j|^2) -- the same bits as one entry
// of the exact distance GEMM.  qrow: row i (LDS or global), grow: row j in global memory.
__device__ __forceinline__ float exact_dist_chain(const float *qrow, const float *__restrict__ grow, int d, float ni, float nj) {
    float acc = 0.0f;
    int k = 0;
    if ((reinterpret_cast<uintptr_t>(grow) & 15) == 0 && d >= 32) {
        // one 128-byte line of row j per batch (8 x 16 B issued back to back: the lanes of a wave walk 64 different
        // rows, so a batch touches 64 lines once), the next batch in flight while this one feeds the chain
        float4 nx[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) nx[u] = *reinterpret_cast<const float4 *>(grow + 4 * u);
        const int nb = d >> 5;
        for (int b = 0; b < nb; ++b) {
            float4 cur[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) cur[u] = nx[u];
            if (b + 1 < nb) {
#pragma unroll
                for (int u = 0; u < 8; ++u) nx[u] = *reinterpret_cast<const float4 *>(grow + (b + 1) * 32 + 4 * u);
            }
            const float *qk = qrow + b * 32;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                acc = fmaf(qk[4 * u + 0], cur[u].x, acc);
                acc = fmaf(qk[4 * u + 1], cur[u].y, acc);
                acc = fmaf(qk[4 * u + 2], cur[u].z, acc);
                acc = fmaf(qk[4 * u + 3], cur[u].w, acc);
            }
        }
        k = nb << 5;
    }
    for (; k < d; ++k) acc = fmaf(qrow[k], grow[k], acc);
    return fmaf(-2.0f, acc, ni + nj);
}

// Wave-cooperative form of exact_dist_chain: lane l receives the exact distance of row i (qrow, in LDS) to ITS
// candidate row jl (jl < 0: none).  The 64 candidate rows are fetched 32 floats at a time with COALESCED loads (8
// lanes take one 128-byte line of one candidate; a per-lane walk of its own row costs 64 tag look-ups per load
// instruction and ran the texture path at ~0.4 requests per clock), laid into a wave-private LDS tile [64][36] and
// read back by the owning lane, whose fmaf chain therefore keeps the oracle's k-ascending order.  The loads of the next
// 32 floats are in flight while the current ones feed the chain.  tile: 64 * 36 floats of LDS per wave.
constexpr int WXD_STRIDE = 36;
__device__ __forceinline__ float wave_exact_dists(const float *qrow, const float *__restrict__ feat, int d, int jl, float ni,
                                                  const float *__restrict__ sqn, float *tile, int lane) {
    float acc = 0.0f;
    int k0 = 0;
    const bool fast = (d % 4 == 0) && ((reinterpret_cast<uintptr_t>(feat) & 15) == 0) && d >= 32;
    if (fast) {
        const int piece = lane & 7, sub = lane >> 3;
        const float *src[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int jc = __shfl(jl, 8 * u + sub, 64);
            src[u] = (jc >= 0) ? feat + (int64_t)jc * d + piece * 4 : nullptr;
        }
        const int nb = d >> 5;
        float4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = src[u] ? *reinterpret_cast<const float4 *>(src[u]) : make_float4(0.f, 0.f, 0.f, 0.f);
        for (int b = 0; b < nb; ++b) {
#pragma unroll
            for (int u = 0; u < 8; ++u) *reinterpret_cast<float4 *>(tile + (8 * u + sub) * WXD_STRIDE + piece * 4) = v[u];
            if (b + 1 < nb) {
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    v[u] = src[u] ? *reinterpret_cast<const float4 *>(src[u] + (b + 1) * 32) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const float *qk = qrow + b * 32;
#pragma unroll
            for (int p = 0; p < 8; ++p) {
                const float4 g4 = *reinterpret_cast<const float4 *>(tile + lane * WXD_STRIDE + p * 4);
                acc = fmaf(qk[4 * p + 0], g4.x, acc);
                acc = fmaf(qk[4 * p + 1], g4.y, acc);
                acc = fmaf(qk[4 * p + 2], g4.z, acc);
                acc = fmaf(qk[4 * p + 3], g4.w, acc);
            }
            __builtin_amdgcn_wave_barrier();
        }
        k0 = nb << 5;
    }
    if (jl < 0) return 0.0f;
    const float *grow = feat + (int64_t)jl * d;
    for (int k = k0; k < d; ++k) acc = fmaf(qrow[k], grow[k], acc);
    return fmaf(-2.0f, acc, ni + sqn[jl]);
}

// ---- host side ----
constexpr int RB_WORDS = 8;                // 32-bit words per row and reciprocity mask (K <= 256)
constexpr size_t LDS_WG_MAX = 160 * 1024;  // LDS of one workgroup on gfx950

// The clamped k's, one definition for every algorithm and every entry point: numpy slicing clamps the neighbour lists when
// N is smaller than k1+1 / k1/2+1 / k2 (utils/reranking.py:53-54,60-62,76); np.mean then averages over min(k2, N) rows.
struct RerankK {
    int K, KR, h, vcap;    // k1 + 1, rank table width max(K, k2), k1/2 + 1, row stride of V -- all clamped to N
    int64_t qcap_bound;    // most entries a row of V_qe can have
};
static inline RerankK clamp_k(int64_t N, int k1, int k2) {
    RerankK k{};
    k.K = (int)std::min<int64_t>(k1 + 1, N);
    k.KR = std::max(k.K, (int)std::min<int64_t>(k2, N));
    k.h = (int)std::min<int64_t>(mpreid_half_k1(k1), N);
    k.vcap = (int)std::min<int64_t>((int64_t)k.K * (1 + k.h), N);
    k.qcap_bound = std::min<int64_t>(N, (int64_t)std::max(k2, 1) * k.vcap);
    return k;
}

// How the Jaccard stage cuts the row space of the blocked inverted index (256 row blocks of rows_per_block rows): a
// workgroup accumulates one chunk of blocks_per_chunk blocks (rch rows of fp16 accumulators in LDS).  A function of N
// only, so that the workspace layouts can reserve the chunk-boundary table ([N][nchunks + 1] u32) the build writes.
struct JaccardPlan {
    int rpb, bpc, nchunks, rch;
    bool wave_form;   // one 64-thread workgroup per (query, chunk) instead of 256 threads
};
JaccardPlan jaccard_plan(int64_t N);   // N = number of INDEXED rows (the gallery rows)
// bytes of the block histograms [256][N] + the chunk-boundary table [N][nchunks + 1]
// (sized for the worst case over the number of indexed rows: nchunks <= 256)
static size_t csc_hist_bytes(int64_t N) { return ((size_t)N * 256 + (size_t)N * 257) * 4 + ((size_t)(N + 1023) / 1024 + 2) * 8; }

struct StageTimer {
    bool on;
    hipStream_t s;
    std::vector<hipEvent_t> ev;
    StageTimer(bool on_, hipStream_t s_) : on(on_), s(s_) {}
    void mark() {
        if (!on) return;
        hipEvent_t e;
        (void)hipEventCreate(&e);
        (void)hipEventRecord(e, s);
        ev.push_back(e);
    }
    float ms(size_t a, size_t b) {
        float m = 0.f;
        if (on && b < ev.size()) (void)hipEventElapsedTime(&m, ev[a], ev[b]);
        return m;
    }
    ~StageTimer() {
        for (auto e : ev) (void)hipEventDestroy(e);
    }
};

// ---- workspace layouts (offsets in bytes; `total` is what the workspace_bytes entry points answer) ----
struct RerankLayout : RerankK {
    int64_t N, ld;
    size_t feat, norms, D, MT, rowmax, rank, rbits, vcnt, vidx, vval, ucnt, qcnt, qidx, qval, ccnt, chist, cptr, crow, cval,
        counters, total;
};
RerankLayout make_layout(int64_t nq, int64_t ng, int d, int k1, int k2, int has_local);

// The twenty buffers of the candidate pipeline, one block in the single-call layout and the whole of the row-sharded
// phase-1 workspace.  The operands cover all n rows (Np = n rounded up to 256, + `slack` rows where a row block is read in
// whole 256-row tiles from any r_lo); everything per row covers the Mp padded rows of the block the call works on.
struct CandBuffers {
    int64_t Np, Nsp, Mp, slack, ld, fb_max;
    int dp;
    size_t sqn, feat16, samp16, sampn, sampD, tlo, thi, eps, cnt_lo, cnt_hi, list_lo, list_hi, gstat, fb_count, fb_rows, fb_feat,
        fb_sqn, fb_D, fb_rowmax, fb_rank;
};
// rows = the rows the call works on (n for the single call), kr = width of the neighbour table
CandBuffers take_cand_buffers(WsCursor &take, int64_t n, int d, int64_t rows, int kr, int64_t slack);

struct Rerank2Layout : RerankK {   // (qcap_bound: at most RR2_QCAP here)
    int64_t N, ld;
    CandBuffers c;
    size_t feat, rowmax, rank, rankd, rbits, vcnt, vidx, vval, ucnt, qcnt, qidx, qval, ccnt, chist, cptr, crow, cval, dq, counters,
        dq_ws, dq_ws_bytes, total;
};
Rerank2Layout make_layout2(int64_t nq, int64_t ng, int d, int k1, int k2, bool split3_rows = false);

struct WideLayout : RerankK {
    int64_t N, ld;
    int fcap, P, nwg, sort_in_lds, rch;
    int64_t qcap;
    size_t feat, norms, D, MT, rowmax, rank, rsort, rpos, sortscr, rcount, vcnt, vidx, vval, wscr, qcnt, qidx, qval, accscr,
        ccnt, cptr, crow, cval, counters, total;
};
WideLayout make_layout_wide(int64_t nq, int64_t ng, int d, int k1, int k2, int has_local);

// ---- rerank_neighbours.hip ----
int launch_original_dist(const float *q, const float *g, int64_t nq, int64_t ng, int d, const float *local, int only_local,
                         float *feat, float *norms, float *D, float *MT, int64_t ld, hipStream_t stream);
int launch_rowmax_topk(const float *MT, int64_t ld, int64_t N, int KR, int64_t rows, float *rowmax, int *rank,
                       hipStream_t stream, const unsigned *row_count = nullptr);
size_t krecip_lds_bytes(bool sparse, int nw, int K, int vcap, int d);   // dynamic LDS of krecip_kernel
int launch_krecip(bool sparse, const float *MT, int64_t ld, int64_t N, const float *rowmax, const int *rank, int K, int KR,
                  int h, int vcap, int *vcnt, int *vidx, uint16_t *vval, int64_t row0, int64_t rows, int *r_count,
                  const float *feat, const float *norms, int d, const float *rankd, unsigned *rk, hipStream_t stream);

// ---- rerank.hip ----
void launch_sum_i32(const int *x, int64_t n, unsigned long long *out, hipStream_t stream);   // out[0] = sum of x[0..n)
void launch_max_i32(const int *x, int64_t n, int *out, hipStream_t stream);                  // out[0] = max of x[0..n)
uint16_t f64_to_f16_host(double d);
// the atomic-cursor index build (row stride and offsets are 64-bit there); no launch check: the caller's
int launch_csc_atomic(int64_t N, int64_t nq, const int *fcnt, const int *fidx, const uint16_t *fval, int fcap, unsigned *ccnt,
                      long long *cptr, int *crow, uint16_t *cval, hipStream_t stream);

// ---- rerank_sparse.hip ----
// the candidate pipeline over the rows [r_lo, r_lo + rows) of the n x n problem, in two halves (the single call forks its
// side stream between them); c.sqn holds the squared norms of all n rows, zero padded, when cand_lists is called
int cand_lists(const float *feat, char *ws, const CandBuffers &c, int64_t n, int d, int64_t r_lo, int64_t rows, int sym,
               int stagger, hipStream_t stream);
int cand_refine(const float *feat, char *ws, const CandBuffers &c, int64_t n, int d, int kr, int64_t r_lo, int64_t rows,
                float *rowmax, int *rank, float *rankd, hipStream_t stream);
bool sparse_eligible(int64_t nq, int64_t ng, int k1, int k2, const float *local);
int rerank_sparse(const float *q, const float *g, int64_t nq, int64_t ng, int d, int k1, int k2, double lambda_value,
                  float *out, int64_t ldo, void *ws, size_t ws_bytes, mpreid_stream_t stream_, mpreid_rerank_stats *stats,
                  int timing, bool split3_rows);

// ---- rerank_wide.hip ----
bool wide_fits(int64_t nq, int64_t ng);
int rerank_wide(const float *q, const float *g, int64_t nq, int64_t ng, int d, int k1, int k2, double lambda_value,
                const float *local, int only_local, float *out, int64_t ldo, void *ws, size_t ws_bytes,
                mpreid_stream_t stream_, mpreid_rerank_stats *stats, int timing);

// Everything after the V rows (query expansion, inverted index, Jaccard + blend, statistics): shared by the dense and
// the sparse algorithm.  MT = distance rows of (at least) the queries, row stride ld; rowmax indexed like MT's rows.
// The ONE host round trip of the call is in here: 16 bytes (largest union size of the query expansion, which sizes
// the ELL rows of V_qe and the LDS of the kernels that walk them, and nnz(V)); counts and sums are reduced on the GPU.
struct TailArgs {
    int64_t N, nq;
    int k1, k2, KR, h, vcap;
    int64_t qcap_bound;   // capacity the workspace was sized for (entries per row of V_qe / of the inverted index)
    const int *rank;
    int *vcnt, *vidx;
    uint16_t *vval;
    int *ucnt, *qcnt, *qidx;
    uint16_t *qval;
    unsigned *ccnt;
    unsigned *chist;                // [CSC_B][N] block histograms of the atomics-free inverted-index build (or NULL)
    long long *cptr;
    int *crow;
    uint16_t *cval;
    unsigned long long *counters;   // [0] Jaccard pairs, [1] sum |R|, [2] nnz(V), [3] max union (int), [4] fallback rows, [5] candidates, [6] nnz(V_qe)
    const float *MT;
    int64_t ld;
    const float *rowmax;
    float *out;
    int64_t ldo;
    double lambda_value;
    int algo;
    hipEvent_t join;   // (sparse) the distance rows MT are produced on a side stream: the Jaccard stage waits for this
    // (sparse, no side stream) launches the exact distance rows on the main stream; the tail calls it BETWEEN the
    // device-side sizing of the V_qe rows and the host's wait for that size, so that the host round trip happens while
    // the GPU works on the rows instead of leaving a ~40 us bubble
    std::function<int(hipStream_t)> mid_launch;
    hipEvent_t sized;   // recorded after the size has been copied to the host buffer
};
int rerank_tail(const TailArgs &a, hipStream_t stream, StageTimer &tm, mpreid_rerank_stats *stats, int marks_so_far);
void fill_rerank_stats(mpreid_rerank_stats *stats, int64_t N, int k1, int k2, int h, int vcap, int vqe_cap,
                       const unsigned long long cnt[7], int algo, StageTimer &tm, int qe0, int dq0, int dq1, int csc0,
                       bool timed_dq);
