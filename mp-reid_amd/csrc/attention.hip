// attention.hip — every attention kernel of the towers for gfx950, behind the four dispatchers of attention.h:
//   attention_kernel / attention_split_kernel (L <= 256, K / V of a head in LDS), attention_long_kernel (streamed K / V),
//   attention_f32_kernel / attention_f32_chunked_kernel (the all-fp32 mode), attention_causal_kernel (the text tower),
// and the unit seams mpreid_vit_attention / mpreid_vit_attention_f32 / mpreid_text_attention of include/mpreid.h.
// Compiled with the flags of vit.hip (mpreid/build.py EXTRA_FLAGS): the kernels rely on -ffinite-math-only.
#include "attention.h"
#include "gemm_f16.h"
#include "towers.h"

// ---------------------------------------------------------------------------------------------
// attention: softmax(q k^T / sqrt(64)) v per (image, head); L <= 16*KTP keys live in LDS.
//
// One workgroup per (image, head); each wave owns 16-query tiles.  Computed "key on the lane":
//   S^T = K Q^T   (A = K rows from LDS, B = Q fragment straight from global)  -> C: col = query
//   O^T = V^T P^T (A = V^T from LDS,   B = P^T = the S^T accumulators, converted in registers)
// so the softmax reduction over keys is in-lane + 2 shuffles and P never touches LDS
// (cdna_hip_programming.md §3 "An accumulator tile as the next MFMA's operand").
// ---------------------------------------------------------------------------------------------
typedef _Float16 h4_t __attribute__((ext_vector_type(4)));

// K / V prefetch registers are NAMED scalars (k0..k4, v0..v4) expanded by macros: as arrays they were kept
// in scratch memory by hipcc, doubling the memory traffic of the kernel.
// thread -> (row, 16-byte chunk), 8 lanes per 128-byte row, so every wave instruction covers 8 whole cache
// lines.  Rows past L are clamped (always a valid address): a guarded load would put every load in its own
// branch with a vmcnt(0) behind it; clamped copies are harmless because keys >= L are masked before softmax.
#define ATT_FOR_EACH_ITER(X) X(0) X(1) X(2) X(3) X(4)
// K / V are read exactly once and O is read only by a later kernel: streaming loads / stores keep them from evicting
// the operand panels of the GEMMs that run beside this kernel on other streams
typedef unsigned att_u4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 load_nt16(const _Float16 *p) {
    const att_u4 v = __builtin_nontemporal_load(reinterpret_cast<const att_u4 *>(p));
    return make_uint4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ void store_nt16(_Float16 *p, const uint4 &v) {
    const att_u4 nv = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(nv, reinterpret_cast<att_u4 *>(p));
}
#define ATT_DECL(i) uint4 k##i = make_uint4(0, 0, 0, 0), v##i = k##i;
#define ATT_LOAD(i)                                                                                  \
    if constexpr (K_ITERS > i) {                                                                     \
        const int idx_ = tid + i * NT;                                                               \
        const int row_ = idx_ >> 3, c_ = idx_ & 7;                                                   \
        const int rc_ = row_ < L ? row_ : L - 1;                                                     \
        k##i = load_nt16(pbase_ + (int64_t)rc_ * ld + W + c_ * 8);                                   \
        v##i = load_nt16(pbase_ + (int64_t)rc_ * ld + 2 * W + c_ * 8);                               \
    }
#define ATT_STORE(i)                                                                                 \
    if constexpr (K_ITERS > i) {                                                                     \
        const int idx_ = tid + i * NT;                                                               \
        const int row_ = idx_ >> 3, c_ = idx_ & 7;                                                   \
        if (idx_ < KEYS * 8) {                                                                       \
            *reinterpret_cast<uint4 *>(Ks + row_ * 128 + ((c_ ^ (row_ & 7)) << 4)) = k##i;           \
            *reinterpret_cast<uint4 *>(Vs + row_ * 128 + ((c_ ^ (((row_ >> 1) & 3) << 1)) << 4)) = v##i; \
        }                                                                                            \
    }
#define ATT_PREFETCH(pr)                                                                             \
    {                                                                                                \
        const int pb_ = (pr) / heads, ph_ = (pr) - pb_ * heads;                                      \
        const _Float16 *pbase_ = qkv + (int64_t)pb_ * L * ld + ph_ * 64;                             \
        ATT_FOR_EACH_ITER(ATT_LOAD)                                                                  \
    }

// All-reduce over the lanes l, l^16, l^32, l^48 (the four key groups of a query column) with gfx950's
// v_permlane16_swap / v_permlane32_swap: with both operands = x, the two results hold (own, partner) in one order or the
// other for every lane, so op(r[0], r[1]) is the xor-16 (then xor-32) exchange -- two VALU operations per step where
// __shfl_xor compiles to ds_bpermute_b32 (an LDS crossbar round trip, ~120 cycles; four per query tile).  Same bits: the
// operations are commutative.
__device__ __forceinline__ float xor16_32_max(float x) {
    auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    x = fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
    r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float xor16_32_sum(float x) {
    auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    x = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

typedef short att_s4 __attribute__((__vector_size__(4 * sizeof(short))));
typedef __attribute__((address_space(3))) att_s4 att_lds_s4;

// Persistent form: a workgroup walks (image, head) pairs pair = blockIdx.x, + gridDim.x, ...  The
// K / V / Q data of the NEXT pair are requested into registers before the current pair is computed
// from LDS, so HBM loads stay in flight during the MFMA/softmax phase (the non-persistent form kept
// loads in flight only about half of the time: 2.5 TB/s).
template <int KTP, int NW, bool EXACT>
__global__ __launch_bounds__(64 * NW, (NW == 8 && KTP <= 10) ? 4 : 2) void attention_kernel(const _Float16 *__restrict__ qkv, int L, int W, int heads,
                                                               _Float16 *__restrict__ out, int q_tiles,
                                                               int total_pairs, int dbg_) {
#ifdef MPREID_ABLATION
    const int dbg = dbg_;
#else
    constexpr int dbg = 0;   // (see attention_split_kernel)
    (void)dbg_;
#endif
    constexpr int KEYS = KTP * 16;
    constexpr int NT = 64 * NW;
    constexpr int K_ITERS = (KEYS * 8 + NT - 1) / NT;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // K  [KEYS][128 B], 16-byte chunk ^= row & 7           (ds_read_b128 of A fragments, conflict free)
    // V  [KEYS][128 B], 16-byte chunk ^= ((row>>1)&3) << 1 (ds_read_b64_tr_b16 of 4-key x 16-d blocks, conflict free)
    unsigned char *Ks = smem;
    unsigned char *Vs = smem + KEYS * 128;
    constexpr int OS = 72;                                                // halfs per row of an O patch (144 B)
    _Float16 *Ot = reinterpret_cast<_Float16 *>(smem + 2 * KEYS * 128);   // [NW][16][OS]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    const int64_t ld = 3 * (int64_t)W;
    const int nqt = (q_tiles > 0) ? q_tiles : (L + 15) / 16;
    const float scale_log2e = 0.125f * 1.44269504088896340736f;

    static_assert(K_ITERS <= 5, "extend ATT_FOR_EACH_ITER");
    ATT_FOR_EACH_ITER(ATT_DECL)

    int pair = blockIdx.x;
    if (pair >= total_pairs) return;
    if (!(dbg & 1)) ATT_PREFETCH(pair)
    for (; pair < total_pairs; pair += gridDim.x) {
        const int b = pair / heads, h = pair - b * heads;
        const _Float16 *base = qkv + (int64_t)b * L * ld + h * 64;
        __syncthreads(); // every wave is done reading the previous pair from LDS
        // ---- registers -> LDS (rows >= L hold a clamped, finite copy of row L-1: masked before the softmax) ----
        ATT_FOR_EACH_ITER(ATT_STORE)
        f16x8 qf[2];
        {   // Q fragment (B operand: B[k = d][col = query]) of this wave's first tile, requested before the
            // barrier; rows past L are clamped and only feed discarded output columns
            const int q = wave * 16 + fr;
            const int qc = q < L ? q : L - 1;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
                qf[ks] = *reinterpret_cast<const f16x8 *>(base + (int64_t)qc * ld + ks * 32 + fq * 8);
        }
        __syncthreads();
        {   // unconditional (a clamped pair index on the last trip): keeps the register arrays out of scratch
            const int nxt = pair + (int)gridDim.x < total_pairs ? pair + (int)gridDim.x : pair;
            if (!(dbg & 1)) ATT_PREFETCH(nxt)
        }

        for (int qt = wave; qt < ((dbg & 2) ? 0 : nqt); qt += NW) {
            const int q = qt * 16 + fr;
            if (qt != wave) { // later tiles of this wave (only when there are more tiles than waves)
                const int qc = q < L ? q : L - 1;
#pragma unroll
                for (int ks = 0; ks < 2; ++ks)
                    qf[ks] = *reinterpret_cast<const f16x8 *>(base + (int64_t)qc * ld + ks * 32 + fq * 8);
            }
        // S^T tiles, branch free.  EXACT: KTP is the even round-up of ceil(L/16), so tiles 0..KTP-3
        // hold only valid keys and only the last two can contain keys >= L (K rows past L are zero in
        // LDS; their scores are forced to -huge).  !EXACT (KTP larger than needed): mask every tile.
        f32x4 s[KTP];
        float mx = -3.0e38f;
#pragma unroll
        for (int kt = 0; kt < KTP; ++kt) {
            s[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const f16x8 kf = *reinterpret_cast<const f16x8 *>(Ks + (kt * 16 + fr) * 128 +
                                                                   (((ks * 4 + fq) ^ (lane & 7)) << 4));
                s[kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, qf[ks], s[kt], 0, 0, 0);
            }
            // keep at most two tiles' worth of K fragments in flight (bounds the register live ranges
            // so that two workgroups fit a CU)
            if (kt & 1) __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int kt = 0; kt < KTP; ++kt) {
            if (!EXACT || kt >= KTP - 2) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (kt * 16 + fq * 4 + r >= L) s[kt][r] = -3.0e38f;
            }
            mx = fmaxf(mx, fmaxf(fmaxf(s[kt][0], s[kt][1]), fmaxf(s[kt][2], s[kt][3])));
        }
        mx = xor16_32_max(mx);
        // p = exp2(s*c - mx*c): one fma + one v_exp per element; masked entries give exp2(-huge) = 0
        const float nmx = -mx * scale_log2e;
        float sum = 0.f;
#pragma unroll
        for (int kt = 0; kt < KTP; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = __builtin_amdgcn_exp2f(fmaf(s[kt][r], scale_log2e, nmx));
                s[kt][r] = p;
                sum += p;
            }
        sum = xor16_32_sum(sum);
        // O^T = V^T P^T over 32-key steps; P^T fragment element j <-> key 32*s2 + 16*(j>>2) + 4*fq + (j&3)
        // (V^T columns past L are zero in LDS and their P is 0, so every step runs unconditionally)
        f32x4 o[4];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s2 = 0; s2 < KTP / 2; ++s2) {
            f16x8 pf;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                pf[j] = (_Float16)s[2 * s2][j];
                pf[4 + j] = (_Float16)s[2 * s2 + 1][j];
            }
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                // A operand = V^T: lane (d = dt*16 + fr, key group fq) needs keys 32*s2 + 4*fq + {0..3} and + 16.
                // One ds_read_b64_tr_b16 hands lane i of a 16-lane group column i of a 4-row x 16-column block;
                // lane 4q+p of the group supplies the address of row q, columns 4p..4p+3.
                const int trq = fr >> 2, trp = fr & 3;
                const int row0 = s2 * 32 + fq * 4 + trq;
                const int chunk = dt * 2 + (trp >> 1);
                const unsigned char *a0 = Vs + row0 * 128 + ((chunk ^ (((row0 >> 1) & 3) << 1)) << 4) + (trp & 1) * 8;
                const int row1 = row0 + 16;
                const unsigned char *a1 = Vs + row1 * 128 + ((chunk ^ (((row1 >> 1) & 3) << 1)) << 4) + (trp & 1) * 8;
                const att_s4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((att_lds_s4 *)a0);
                const att_s4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((att_lds_s4 *)a1);
                typedef short s8_t __attribute__((ext_vector_type(8)));
                const s8_t vs8 = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                const f16x8 vf = __builtin_bit_cast(f16x8, vs8);
                o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf, pf, o[dt], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        // O^T accumulators hold 4 consecutive d for one query per lane.  Writing them straight out would be
        // 8-byte stores touching 16 partial lines per instruction (store-issue-bound); instead the wave's
        // 16 x 64 tile goes through its private LDS patch and leaves as whole 128-byte rows, 16 B per lane.
        {
            const float inv = 1.0f / sum;
            _Float16 *ot = Ot + wave * (16 * OS);
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                h4_t ov = {(_Float16)(o[dt][0] * inv), (_Float16)(o[dt][1] * inv), (_Float16)(o[dt][2] * inv),
                           (_Float16)(o[dt][3] * inv)};
                *reinterpret_cast<h4_t *>(ot + fr * OS + dt * 16 + fq * 4) = ov;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
            for (int it = 0; it < 2; ++it) {
                const int row = it * 8 + (lane >> 3), ch = lane & 7;
                const uint4 v = *reinterpret_cast<const uint4 *>(ot + row * OS + ch * 8);
                const int qrow = qt * 16 + row;
                if (qrow < L && !(dbg & 4))
                    store_nt16(out + ((int64_t)b * L + qrow) * W + h * 64 + ch * 8, v);
            }
            __builtin_amdgcn_wave_barrier();
        }
        } // query tiles
    }     // (image, head) pairs
}

// ---------------------------------------------------------------------------------------------
// attention of the `split` precision mode: the same "key on the lane" scheme, fp32-grade on the fp16 matrix cores.
// q | k | v arrive as fp32 [M][3W] (GE_S_BIAS_F32); K and V are split into fp16 pairs (hi, lo) while they are staged into
// LDS (Kh, Kl, Vh, Vl: four arrays in the layouts of the fp16 kernel), Q in registers, and every product runs as
// hi.hi' + lo.hi' + hi.lo' into the one fp32 accumulator:
//   S^T = Kh Qh^T + Kl Qh^T + Kh Ql^T          O^T = Vh^T Ph^T + Vl^T Ph^T + Vh^T Pl^T
// The softmax is fp32 in registers as before; P carries a factor 2^10 (added to the exponent, cancelled by the
// division by the row sum, which carries it too) so that the lo parts of small probabilities stay far away from the
// bottom of the fp16 range.  O leaves as the fp16 pair [hi(W) | lo(W)] per row: the A operand of the out-proj GEMM.
// One workgroup per CU (80-128 KB of LDS); persistent over (image, head) pairs with the next pair's K / V prefetched
// into registers, like the fp16 kernel.
// ---------------------------------------------------------------------------------------------
typedef float att_f4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 load_nt_f4(const float *p) {
    const att_f4 v = __builtin_nontemporal_load(reinterpret_cast<const att_f4 *>(p));
    return make_float4(v[0], v[1], v[2], v[3]);
}
typedef unsigned att_u4 __attribute__((ext_vector_type(4)));
// 16 bytes through a buffer descriptor: base in scalar registers, 32-bit lane offset, scalar offset (both in bytes); nt
template <typename RS>
__device__ __forceinline__ float4 buffer_load_nt_f4(const RS &rs, unsigned voff, int soff) {
    const att_f4 v = __builtin_bit_cast(att_f4, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)voff, soff, 2));
    return make_float4(v[0], v[1], v[2], v[3]);
}
template <typename RS>
__device__ __forceinline__ float4 buffer_load_f4(const RS &rs, unsigned voff, int soff) {   // the same, cached as a plain load
    const att_f4 v = __builtin_bit_cast(att_f4, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)voff, soff, 0));
    return make_float4(v[0], v[1], v[2], v[3]);
}
template <typename RS>
__device__ __forceinline__ void buffer_store_nt16(const RS &rs, unsigned voff, int soff, const uint4 &v) {
    const att_u4 nv = {v.x, v.y, v.z, v.w};
    __builtin_amdgcn_raw_buffer_store_b128(nv, rs, (int)voff, soff, 2);
}
__device__ __forceinline__ void split4(const float4 &v, h4_t &hi, h4_t &lo) {
    const float x[4] = {v.x, v.y, v.z, v.w};
    split_pairs<4>(x, hi, lo);   // (common.h: three instructions per two values)
}
#define ATS_FOR_EACH_ITER(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7)
#define ATS_DECL(i) float4 k##i = make_float4(0.f, 0.f, 0.f, 0.f), v##i = k##i; unsigned koff##i = 0u;
// thread -> (row, 16-byte chunk of 4 floats), 16 lanes per 256-byte row; rows past L clamped (see the fp16 kernel).
// The byte offset of a thread's chunk inside an (image, head) slab does not depend on the pair: computed ONCE (ATS_OFFS, a
// 32-bit register per iteration) and every load is a BUFFER load: descriptor of the image's q | k | v slab (scalar registers,
// rebuilt per pair from uniform values), 32-bit lane offset, scalar offset of the head's K / V columns -- no vector ALU work per
// load (the 64-bit per-lane address arithmetic of plain global loads cost three v_lshl_add_u64 each).
#define ATS_OFFS(i)                                                                                  \
    if constexpr (K_ITERS > i) {                                                                     \
        const int idx_ = tid + i * NT;                                                               \
        const int row_ = idx_ >> 4, c_ = idx_ & 15;                                                  \
        const int rc_ = row_ < L ? row_ : L - 1;                                                     \
        koff##i = (unsigned)(rc_ * (int)ld + c_ * 4) * 4u;                                           \
    }
// XKEY (no row is clamped): iteration i is iteration 0 moved down by NT / 16 rows, a uniform distance that goes into the
// scalar offset -- one lane offset register instead of K_ITERS
#define ATS_VOFF(i) (XKEY ? koff0 : koff##i)
#define ATS_SOFF(i) (XKEY ? i * (NT / 16) * (int)ld * 4 : 0)
#define ATS_LOAD(i)                                                                                  \
    if constexpr (K_ITERS > i) {                                                                     \
        k##i = buffer_load_nt_f4(prs_, ATS_VOFF(i), pso_ + ATS_SOFF(i));                             \
        v##i = buffer_load_nt_f4(prs_, ATS_VOFF(i), pso_ + ATS_SOFF(i) + W * 4);                     \
    }
#define ATS_STORE(i)                                                                                 \
    if constexpr (K_ITERS > i) {                                                                     \
        const int idx_ = tid + i * NT;                                                               \
        const int row_ = idx_ >> 4, c_ = idx_ & 15;                                                  \
        if (idx_ < KEYS * 16) {                                                                      \
            h4_t hi_, lo_;                                                                           \
            const int ko_ = row_ * 128 + (((c_ >> 1) ^ (row_ & 7)) << 4) + (c_ & 1) * 8;             \
            split4(k##i, hi_, lo_);                                                                  \
            *reinterpret_cast<h4_t *>(Kh + ko_) = hi_;                                               \
            *reinterpret_cast<h4_t *>(Kl + ko_) = lo_;                                               \
            const int vo_ = row_ * 128 + (((c_ >> 1) ^ (((row_ >> 1) & 3) << 1)) << 4) + (c_ & 1) * 8; \
            split4(v##i, hi_, lo_);                                                                  \
            *reinterpret_cast<h4_t *>(Vh + vo_) = hi_;                                               \
            *reinterpret_cast<h4_t *>(Vl + vo_) = lo_;                                               \
        }                                                                                            \
    }
#define ATS_LOAD_K(i)                                                                                \
    if constexpr (K_ITERS > i) k##i = buffer_load_nt_f4(prs_, ATS_VOFF(i), pso_ + ATS_SOFF(i));
#define ATS_LOAD_V(i)                                                                                \
    if constexpr (K_ITERS > i) v##i = buffer_load_nt_f4(prs_, ATS_VOFF(i), pso_ + ATS_SOFF(i) + W * 4);
// the K rows or the V rows alone (XKEY requests them at two places of the compute phase)
#define ATS_PREFETCH_PART(pr, PART)                                                                  \
    {                                                                                                \
        const int pb_ = (pr) / heads, ph_ = (pr) - pb_ * heads;                                      \
        const auto prs_ = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(qkv + (int64_t)pb_ * L * ld), 0,   \
                                                             (int)(L * (int)ld * 4), 0x00020000);   \
        const int pso_ = (ph_ * 64 + W) * 4;                                                         \
        ATS_FOR_EACH_ITER(PART)                                                                      \
    }
#define ATS_PREFETCH(pr)                                                                             \
    {                                                                                                \
        const int pb_ = (pr) / heads, ph_ = (pr) - pb_ * heads;                                      \
        const auto prs_ = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(qkv + (int64_t)pb_ * L * ld), 0,   \
                                                             (int)(L * (int)ld * 4), 0x00020000);   \
        const int pso_ = (ph_ * 64 + W) * 4;                                                         \
        ATS_FOR_EACH_ITER(ATS_LOAD)                                                                  \
    }

// XKEY (L == 16 * KTP + 1, i.e. ViT-B/16 at 256 x 128: L = 129 = 8 key tiles + ONE token): the tiles cover keys 0 .. L-2
// exactly and the last token is handled as an extra key OUTSIDE the matrix instructions -- its K / V rows sit in LDS as
// fp32 (its Q row beside them: the tail query's operand, staged with them instead of held in registers); its score is 16
// fp32 FMAs per lane on the raw Q values + one cross-group sum, its P x V contribution 16 FMAs on the
// O accumulators.  Without it the one odd key costs two of ten key tiles (the PV step is 32 keys wide): 20 % of the QK
// products, a fifth PV step, 20 % of the softmax and 16 KB of LDS -- and with 64 + 1 KB of K / V pairs instead of 80 a
// 256-thread workgroup fits a CU TWICE, so one workgroup's loads / staging / barriers overlap the other's compute.
template <int KTP, int NW, bool XKEY>
__global__ __launch_bounds__(64 * NW, (NW >= 8 || XKEY) ? 2 : 1) void attention_split_kernel(const float *__restrict__ qkv, int L, int W,
                                                                                   int heads, _Float16 *__restrict__ out,
                                                                                   int q_tiles, int total_pairs, int dbg_) {
    // The timing-ablation switches are compile-time zero in the product build: as a run-time argument `dbg & 32` kept
    // every key tile's score chain behind its own branch (eight basic blocks, each one strictly serial chain of six
    // dependent matrix instructions with the full issue-to-result latency between them) -- with the flag gone the eight
    // independent chains are one block and interleave.
#ifdef MPREID_ABLATION
    const int dbg = dbg_;
#else
    constexpr int dbg = 0;
    (void)dbg_;
#endif
    constexpr int KEYS = KTP * 16;
    constexpr int NT = 64 * NW;
    constexpr int K_ITERS = (KEYS * 16 + NT - 1) / NT;
    static_assert(K_ITERS <= 8, "extend ATS_FOR_EACH_ITER");
    static_assert(!XKEY || KEYS * 16 == K_ITERS * NT, "ATS_SOFF: every staging iteration is whole and below row L - 1");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char *Kh = smem, *Kl = smem + KEYS * 128, *Vh = smem + 2 * KEYS * 128, *Vl = smem + 3 * KEYS * 128;
    constexpr int OS = 72;
    _Float16 *Ot = reinterpret_cast<_Float16 *>(smem + 4 * KEYS * 128);   // [NW][16][OS]
    float *Xk = reinterpret_cast<float *>(smem + 4 * KEYS * 128 + NW * 16 * OS * 2);   // XKEY: [64] K, [64] V, [64] Q row of token L-1 (fp32)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    const int64_t ld = 3 * (int64_t)W;
    const int nqt = (q_tiles > 0) ? q_tiles : (L + 15) / 16;
    const float scale_log2e = 0.125f * 1.44269504088896340736f;

    ATS_FOR_EACH_ITER(ATS_DECL)
    ATS_FOR_EACH_ITER(ATS_OFFS)
    // XKEY: byte offsets inside an image's slab of this lane's Q chunk in the wave's two main tiles (wave, wave + NW) and of
    // its 16-byte piece of the wave's first output tile (row wave * 16 + (lane >> 3), chunk lane & 7)
    unsigned xq_off[2] = {0u, 0u}, xo_off = 0u;
    if constexpr (XKEY) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int q = (wave + t * NW) * 16 + fr;
            xq_off[t] = (unsigned)((q < L ? q : L - 1) * (int)ld + fq * 8) * 4u;
        }
        xo_off = (unsigned)((wave * 16 + (lane >> 3)) * 2 * W + (lane & 7) * 8) * 2u;
    }

    // XKEY: lanes 0-15 of wave 0 hold the K row of token L-1, lanes 16-31 its V row, lanes 32-47 its Q row (the tail query)
    float4 xrow = make_float4(0.f, 0.f, 0.f, 0.f);
    auto x_request = [&](int pr) {
        if constexpr (XKEY) {
            if (tid < 48) {
                const int pb = pr / heads, ph = pr - pb * heads;
                xrow = load_nt_f4(qkv + ((int64_t)pb * L + (L - 1)) * ld + ph * 64 + (tid < 16 ? W : tid < 32 ? 2 * W : 0) + (tid & 15) * 4);
            }
        }
    };
    // dbg (MPREID_ATT_DBG in an MPREID_ABLATION build; timing ablations only, wrong results): 1 no K / V loads, 2 no compute,
    // 4 no output stores, 8 no PV, 16 no O write-out, 32 no QK products.  Ablation of <8,4,XKEY> at B = 508, L = 129 (us per
    // launch, tools/attention_bench.py, profiles/attention_split_ablation.log) with one pass over K / V per query tile:
    // full 210; loads + staging only 85; compute on stale LDS 134; without stores 200, PV 185, O write-out 187, QK 183.
    // With one pass for both of a wave's tiles and the LDS reads a step ahead (xkey_tiles): full 169.
    int pair = blockIdx.x;
    if (pair >= total_pairs) return;
    if (!(dbg & 1)) {
        ATS_PREFETCH(pair)
        x_request(pair);
    }
    for (; pair < total_pairs; pair += gridDim.x) {
        const int b = pair / heads, h = pair - b * heads;
        const float *base = qkv + (int64_t)b * L * ld + h * 64;
        __syncthreads(); // every wave is done reading the previous pair from LDS
        ATS_FOR_EACH_ITER(ATS_STORE)
        if constexpr (XKEY) {
            if (tid < 48) *reinterpret_cast<float4 *>(Xk + tid * 4) = xrow;
        }
        // Q of this wave's first query tile (B operand: B[k = d][col = query]; 8 consecutive d per lane and 32-wide k step),
        // requested BEFORE the barrier so that its round trip is hidden behind it; the next tile's Q (a wave has a second
        // tile only when there are more tiles than waves) is requested while the current tile is computed.  Fetched at the
        // top of each tile instead, every tile started with an exposed global round trip: 289 -> 2xx us per layer-batch.
        float4 qraw[4];
        auto q_request = [&](int qt) {
            const int q = qt * 16 + fr;
            const int qc = q < L ? q : L - 1;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const float *qp = base + (int64_t)qc * ld + ks * 32 + fq * 8;
                qraw[2 * ks] = *reinterpret_cast<const float4 *>(qp);
                qraw[2 * ks + 1] = *reinterpret_cast<const float4 *>(qp + 4);
            }
        };
        // XKEY: Q through the descriptor of the image's q | k | v slab and the output through one of its output slab, both with
        // lane offsets computed once per kernel (xq_off, xo_off) and everything that changes per pair or tile in the scalar
        // offset -- no per-lane 64-bit address arithmetic in the tile body.  A wave's two main tiles (wave, wave + NW) are
        // requested together and computed in ONE pass over K / V (xkey_tiles below).
        float4 qx[2][4];
        const auto xq_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(qkv + (int64_t)b * L * ld), 0, (int)(L * (int)ld * 4),
                                                             0x00020000);
        const auto xo_rs = __builtin_amdgcn_make_buffer_rsrc(out + (int64_t)b * L * 2 * W, 0, (int)(L * 2 * W * 2), 0x00020000);
        auto xq_request = [&](float4 *dst, unsigned voff) {
#pragma unroll
            for (int c = 0; c < 4; ++c) dst[c] = buffer_load_f4(xq_rs, voff, h * 256 + (c >> 1) * 128 + (c & 1) * 16);
        };
        const int x_ntq = !XKEY ? 0 : (wave + NW < (nqt == KTP + 1 ? KTP : nqt) ? 2 : (wave < nqt ? 1 : 0));
        if constexpr (XKEY) {
            if (x_ntq >= 1) xq_request(qx[0], xq_off[0]);
            if (x_ntq == 2) xq_request(qx[1], xq_off[1]);
        } else {
            q_request(wave < nqt ? wave : 0);
        }
        __syncthreads();
        const int nxt = pair + (int)gridDim.x < total_pairs ? pair + (int)gridDim.x : pair;
        // XKEY: the next pair's K / V are requested after the softmax of the wave's tiles (xkey_tiles), when the score
        // registers are dead; a wave without a tile (q_tiles > 0) requests them here
        if (!(dbg & 1) && (!XKEY || x_ntq == 0 || (dbg & 2))) {
            ATS_PREFETCH(nxt)
            x_request(nxt);
        }
        // XKEY, all query tiles wanted: the tiles 0 .. KTP-1 are full, tile KTP holds ONE query (token L-1).  Handed to one
        // wave as a tile of its own (round 3) that wave did three tiles per pair where the others did two, and everybody
        // waited for it at the next barrier: a third of the compute phase for 1/129 of the rows.  Now the waves share it BY
        // KEYS (below, after the main tiles): every wave scores the query against its own two key tiles, the partial
        // (max, sum, O) leave through LDS and wave 0 merges them -- a quarter tile per wave instead of a whole one for one.
        const bool tail = XKEY && nqt == KTP + 1;
        const int nmain = tail ? KTP : nqt;
        // XKEY: the wave's NTQ main tiles (wave, wave + NW) in ONE pass over K / V.  Every K fragment and every transposed V
        // fragment is read from LDS once and multiplied into both tiles' accumulators: half the LDS read bytes and address
        // arithmetic of a pass per tile, and twice as many independent accumulation chains to put between a fragment's
        // read and its use.  Each accumulator sees the products of the single-tile form in the same order (key tile, then
        // ks, then hi.hi' + lo.hi' + hi.lo'; PV step, then dt), the softmax is per tile as before: the bits are the same.
        // The next pair's K (32 registers) is requested after the softmax and its V (32) after the second of the four PV
        // steps, when half of P is consumed, instead of both before the tiles: two tiles' scores fit where one tile's did.
        // The rest of the PV phase, the write-out, the tail query and the barrier cover their round trip.  (Requested
        // earlier -- K at the barrier or before the softmax, V right after the softmax -- 18 to 21 registers spill.)
        auto xkey_tiles = [&](auto ntq_) {
            constexpr int NTQ = decltype(ntq_)::value;
            f16x8 qh[NTQ][2], ql[NTQ][2];
            float sx[NTQ];   // q . k of the extra key (token L-1), fp32, for this lane's query column
#pragma unroll
            for (int t = 0; t < NTQ; ++t) {
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    const float4 a0 = qx[t][2 * ks], a1 = qx[t][2 * ks + 1];
                    const float qv[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
                    split_pairs<8>(qv, qh[t][ks], ql[t][ks]);
                }
                sx[t] = 0.f;
#pragma unroll
                for (int c = 0; c < 4; ++c) {   // this lane's 16 d values: ks * 32 + fq * 8 + (c & 1) * 4 .. + 3
                    const float4 kx = *reinterpret_cast<const float4 *>(Xk + (c >> 1) * 32 + fq * 8 + (c & 1) * 4);
                    sx[t] = fmaf(qx[t][c].x, kx.x, sx[t]);
                    sx[t] = fmaf(qx[t][c].y, kx.y, sx[t]);
                    sx[t] = fmaf(qx[t][c].z, kx.z, sx[t]);
                    sx[t] = fmaf(qx[t][c].w, kx.w, sx[t]);
                }
                sx[t] = xor16_32_sum(sx[t]);
            }
            // the K fragments of step i + 1 (i = 2 kt + ks) are requested before the products of step i are issued, and the
            // scheduler is held to that order (a group of two LDS reads, then the step's 3 NTQ matrix instructions)
            f32x4 s[NTQ][KTP];
            f16x8 kh[2], kl[2];
            auto k_read = [&](int i) {
                const int ko = ((i >> 1) * 16 + fr) * 128 + ((((i & 1) * 4 + fq) ^ (lane & 7)) << 4);
                kh[i & 1] = *reinterpret_cast<const f16x8 *>(Kh + ko);
                kl[i & 1] = *reinterpret_cast<const f16x8 *>(Kl + ko);
            };
            __builtin_amdgcn_sched_barrier(0);   // (the reads of the extra key's row above are no part of the groups below)
            if (!(dbg & 32)) {
                k_read(0);
                __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
            }
#pragma unroll
            for (int i = 0; i < 2 * KTP; ++i) {
                const int kt = i >> 1, ks = i & 1;
                if (ks == 0) {
#pragma unroll
                    for (int t = 0; t < NTQ; ++t) s[t][kt] = f32x4{0.f, 0.f, 0.f, 0.f};
                }
                if (!(dbg & 32)) {
                    if (i + 1 < 2 * KTP) {
                        k_read(i + 1);
                        __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
                    }
#pragma unroll
                    for (int t = 0; t < NTQ; ++t) {
                        s[t][kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kh[i & 1], qh[t][ks], s[t][kt], 0, 0, 0);
                        s[t][kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kl[i & 1], qh[t][ks], s[t][kt], 0, 0, 0);
                        s[t][kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kh[i & 1], ql[t][ks], s[t][kt], 0, 0, 0);
                    }
                    __builtin_amdgcn_sched_group_barrier(0x8, 3 * NTQ, 0);
                }
            }
            float sum[NTQ], px[NTQ];
#pragma unroll
            for (int t = 0; t < NTQ; ++t) {
                float mx = -3.0e38f;
#pragma unroll
                for (int kt = 0; kt < KTP; ++kt)
                    mx = fmaxf(mx, fmaxf(fmaxf(s[t][kt][0], s[t][kt][1]), fmaxf(s[t][kt][2], s[t][kt][3])));
                mx = xor16_32_max(mx);
                mx = fmaxf(mx, sx[t]);
                // p * 2^10 = exp2(s*c - mx*c + 10)
                const float nmx = fmaf(-mx, scale_log2e, 10.0f);
                sum[t] = 0.f;
#pragma unroll
                for (int kt = 0; kt < KTP; ++kt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float p = __builtin_amdgcn_exp2f(fmaf(s[t][kt][r], scale_log2e, nmx));
                        s[t][kt][r] = p;
                        sum[t] += p;
                    }
                sum[t] = xor16_32_sum(sum[t]);
                px[t] = __builtin_amdgcn_exp2f(fmaf(sx[t], scale_log2e, nmx));
                sum[t] += px[t];
            }
            __builtin_amdgcn_sched_barrier(0);
            if (!(dbg & 1)) {
                ATS_PREFETCH_PART(nxt, ATS_LOAD_K)
                x_request(nxt);
            }
            __builtin_amdgcn_sched_barrier(0);
            f32x4 o[NTQ][4];
#pragma unroll
            for (int t = 0; t < NTQ; ++t)
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) o[t][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
            // the transposed V fragments of step j + 1 (j = 4 s2 + dt) are requested before the products of step j, like K
            f16x8 vh[2], vl[2];
            auto v_read = [&](int j) {
                const int trq = fr >> 2, trp = fr & 3;
                const int row0 = (j >> 2) * 32 + fq * 4 + trq, row1 = row0 + 16;
                const int chunk = (j & 3) * 2 + (trp >> 1);
                const int o0 = row0 * 128 + ((chunk ^ (((row0 >> 1) & 3) << 1)) << 4) + (trp & 1) * 8;
                const int o1 = row1 * 128 + ((chunk ^ (((row1 >> 1) & 3) << 1)) << 4) + (trp & 1) * 8;
                typedef short s8_t __attribute__((ext_vector_type(8)));
                const att_s4 h0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((att_lds_s4 *)(Vh + o0));
                const att_s4 h1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((att_lds_s4 *)(Vh + o1));
                const att_s4 l0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((att_lds_s4 *)(Vl + o0));
                const att_s4 l1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((att_lds_s4 *)(Vl + o1));
                const s8_t vh8 = {h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]};
                const s8_t vl8 = {l0[0], l0[1], l0[2], l0[3], l1[0], l1[1], l1[2], l1[3]};
                vh[j & 1] = __builtin_bit_cast(f16x8, vh8);
                vl[j & 1] = __builtin_bit_cast(f16x8, vl8);
            };
            if (!(dbg & 8)) {
                v_read(0);
                __builtin_amdgcn_sched_group_barrier(0x100, 4, 1);
            }
#pragma unroll
            for (int s2 = 0; s2 < ((dbg & 8) ? 0 : KTP / 2); ++s2) {
                f16x8 ph[NTQ], pl[NTQ];
#pragma unroll
                for (int t = 0; t < NTQ; ++t) {
                    const float pv[8] = {s[t][2 * s2][0], s[t][2 * s2][1], s[t][2 * s2][2], s[t][2 * s2][3],
                                         s[t][2 * s2 + 1][0], s[t][2 * s2 + 1][1], s[t][2 * s2 + 1][2], s[t][2 * s2 + 1][3]};
                    split_pairs<8>(pv, ph[t], pl[t]);
                }
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) {
                    const int j = s2 * 4 + dt;
                    // (the read ahead stays on this side of the V request in the middle of the PV steps: full fences there)
                    if (j + 1 < 2 * KTP && !(dt == 3 && s2 == KTP / 4 - 1)) {
                        v_read(j + 1);
                        __builtin_amdgcn_sched_group_barrier(0x100, 4, 1);
                    }
#pragma unroll
                    for (int t = 0; t < NTQ; ++t) {
                        o[t][dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vh[j & 1], ph[t], o[t][dt], 0, 0, 0);
                        o[t][dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vl[j & 1], ph[t], o[t][dt], 0, 0, 0);
                        o[t][dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vh[j & 1], pl[t], o[t][dt], 0, 0, 0);
                    }
                    __builtin_amdgcn_sched_group_barrier(0x8, 3 * NTQ, 1);
                }
                if (s2 == KTP / 4 - 1) {   // half of P is consumed: its registers take the next pair's V
                    __builtin_amdgcn_sched_barrier(0);
                    if (!(dbg & 1)) ATS_PREFETCH_PART(nxt, ATS_LOAD_V)
                    __builtin_amdgcn_sched_barrier(0);
                    v_read(4 * (s2 + 1));
                    __builtin_amdgcn_sched_group_barrier(0x100, 4, 1);
                }
            }
            if ((dbg & 8) && !(dbg & 1)) ATS_PREFETCH_PART(nxt, ATS_LOAD_V)
#pragma unroll
            for (int t = 0; t < NTQ; ++t) {
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) {   // + p_x * v_x: lane (query fr) owns d = dt * 16 + fq * 4 .. + 3
                    const float4 vx = *reinterpret_cast<const float4 *>(Xk + 64 + dt * 16 + fq * 4);
                    o[t][dt][0] = fmaf(px[t], vx.x, o[t][dt][0]);
                    o[t][dt][1] = fmaf(px[t], vx.y, o[t][dt][1]);
                    o[t][dt][2] = fmaf(px[t], vx.z, o[t][dt][2]);
                    o[t][dt][3] = fmaf(px[t], vx.w, o[t][dt][3]);
                }
                if (!(dbg & 16)) {   // O^T -> fp16 pair, through the wave's LDS patch as whole 128-byte rows: hi part, then lo part
                    const float inv = 1.0f / sum[t];
                    _Float16 *ot = Ot + wave * (16 * OS);
                    h4_t ohi[4], olo[4];
#pragma unroll
                    for (int dt = 0; dt < 4; ++dt) {
                        const float ovf[4] = {o[t][dt][0] * inv, o[t][dt][1] * inv, o[t][dt][2] * inv, o[t][dt][3] * inv};
                        split_pairs<4>(ovf, ohi[dt], olo[dt]);
                    }
#pragma unroll
                    for (int part = 0; part < 2; ++part) {
#pragma unroll
                        for (int dt = 0; dt < 4; ++dt)
                            *reinterpret_cast<h4_t *>(ot + fr * OS + dt * 16 + fq * 4) = part == 0 ? ohi[dt] : olo[dt];
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                        __builtin_amdgcn_wave_barrier();
                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
                        for (int it = 0; it < 2; ++it) {
                            const int row = it * 8 + (lane >> 3), ch = lane & 7;
                            const uint4 v = *reinterpret_cast<const uint4 *>(ot + row * OS + ch * 8);
                            // (rows (wave + t * NW) * 16 + it * 8 + (lane >> 3) < 16 * KTP = L - 1: every main-tile row exists)
                            if (!(dbg & 4))
                                buffer_store_nt16(xo_rs, xo_off, ((t * NW * 16 + it * 8) * 2 * W + part * W + h * 64) * 2, v);
                        }
                        __builtin_amdgcn_wave_barrier();
                    }
                }
            }
        };
        if constexpr (XKEY) {
            if (!(dbg & 2)) {
                if (x_ntq == 2) xkey_tiles(std::integral_constant<int, 2>{});
                else if (x_ntq == 1) xkey_tiles(std::integral_constant<int, 1>{});
            }
        }
        if constexpr (!XKEY)
        for (int qt = wave; qt < ((dbg & 2) ? 0 : nmain); qt += NW) {
            f16x8 qh[2], ql[2];
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const float4 a0 = qraw[2 * ks], a1 = qraw[2 * ks + 1];
                const float qv[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
                split_pairs<8>(qv, qh[ks], ql[ks]);
            }
            if (qt + NW < nmain) q_request(qt + NW);
            f32x4 s[KTP];
            float mx = -3.0e38f;
            const int nkt = (L + 15) >> 4;   // key tiles that hold a valid key
#pragma unroll
            for (int kt = 0; kt < KTP; ++kt) {
                s[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (kt < nkt && !(dbg & 32)) {
#pragma unroll
                    for (int ks = 0; ks < 2; ++ks) {
                        const int ko = (kt * 16 + fr) * 128 + (((ks * 4 + fq) ^ (lane & 7)) << 4);
                        const f16x8 kh = *reinterpret_cast<const f16x8 *>(Kh + ko);
                        const f16x8 kl = *reinterpret_cast<const f16x8 *>(Kl + ko);
                        s[kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kh, qh[ks], s[kt], 0, 0, 0);
                        s[kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kl, qh[ks], s[kt], 0, 0, 0);
                        s[kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kh, ql[ks], s[kt], 0, 0, 0);
                    }
                }
                if (kt & 1) __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int kt = 0; kt < KTP; ++kt) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (kt * 16 + fq * 4 + r >= L) s[kt][r] = -3.0e38f;
                mx = fmaxf(mx, fmaxf(fmaxf(s[kt][0], s[kt][1]), fmaxf(s[kt][2], s[kt][3])));
            }
            mx = xor16_32_max(mx);
            // p * 2^10 = exp2(s*c - mx*c + 10); masked entries give exp2(-huge) = 0
            const float nmx = fmaf(-mx, scale_log2e, 10.0f);
            float sum = 0.f;
#pragma unroll
            for (int kt = 0; kt < KTP; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float p = __builtin_amdgcn_exp2f(fmaf(s[kt][r], scale_log2e, nmx));
                    s[kt][r] = p;
                    sum += p;
                }
            sum = xor16_32_sum(sum);
            f32x4 o[4];
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s2 = 0; s2 < ((dbg & 8) ? 0 : KTP / 2); ++s2) {
                f16x8 ph, pl;
                {
                    const float pv[8] = {s[2 * s2][0], s[2 * s2][1], s[2 * s2][2], s[2 * s2][3],
                                         s[2 * s2 + 1][0], s[2 * s2 + 1][1], s[2 * s2 + 1][2], s[2 * s2 + 1][3]};
                    split_pairs<8>(pv, ph, pl);
                }
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) {
                    const int trq = fr >> 2, trp = fr & 3;
                    const int row0 = s2 * 32 + fq * 4 + trq, row1 = row0 + 16;
                    const int chunk = dt * 2 + (trp >> 1);
                    const int o0 = row0 * 128 + ((chunk ^ (((row0 >> 1) & 3) << 1)) << 4) + (trp & 1) * 8;
                    const int o1 = row1 * 128 + ((chunk ^ (((row1 >> 1) & 3) << 1)) << 4) + (trp & 1) * 8;
                    typedef short s8_t __attribute__((ext_vector_type(8)));
                    const att_s4 h0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((att_lds_s4 *)(Vh + o0));
                    const att_s4 h1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((att_lds_s4 *)(Vh + o1));
                    const att_s4 l0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((att_lds_s4 *)(Vl + o0));
                    const att_s4 l1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((att_lds_s4 *)(Vl + o1));
                    const s8_t vh8 = {h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]};
                    const s8_t vl8 = {l0[0], l0[1], l0[2], l0[3], l1[0], l1[1], l1[2], l1[3]};
                    const f16x8 vh = __builtin_bit_cast(f16x8, vh8), vl = __builtin_bit_cast(f16x8, vl8);
                    o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vh, ph, o[dt], 0, 0, 0);
                    o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vl, ph, o[dt], 0, 0, 0);
                    o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vh, pl, o[dt], 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            if (!(dbg & 16)) {   // O^T -> fp16 pair, through the wave's LDS patch as whole 128-byte rows: hi part, then lo part
                const float inv = 1.0f / sum;
                _Float16 *ot = Ot + wave * (16 * OS);
                h4_t ohi[4], olo[4];   // both halves once (split_pairs: three instructions per two values)
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) {
                    const float ovf[4] = {o[dt][0] * inv, o[dt][1] * inv, o[dt][2] * inv, o[dt][3] * inv};
                    split_pairs<4>(ovf, ohi[dt], olo[dt]);
                }
#pragma unroll
                for (int part = 0; part < 2; ++part) {
#pragma unroll
                    for (int dt = 0; dt < 4; ++dt)
                        *reinterpret_cast<h4_t *>(ot + fr * OS + dt * 16 + fq * 4) = part == 0 ? ohi[dt] : olo[dt];
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
                    for (int it = 0; it < 2; ++it) {
                        const int row = it * 8 + (lane >> 3), ch = lane & 7;
                        const uint4 v = *reinterpret_cast<const uint4 *>(ot + row * OS + ch * 8);
                        const int qrow = qt * 16 + row;
                        if (qrow < L && !(dbg & 4)) store_nt16(out + ((int64_t)b * L + qrow) * 2 * W + part * W + h * 64 + ch * 8, v);
                    }
                    __builtin_amdgcn_wave_barrier();
                }
            }
        } // query tiles
        if constexpr (XKEY) {
            if (tail && !(dbg & 2)) {
                static_assert(!XKEY || KTP == 2 * NW, "the tail query is shared by keys: two key tiles (one PV step) per wave");
                // Q of token L-1 was staged into LDS beside the extra key's K / V rows: this lane's 16 d values, as a main
                // tile's lane holds them (every column of this tile is the one query)
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    qraw[c] = *reinterpret_cast<const float4 *>(Xk + 128 + (c >> 1) * 32 + fq * 8 + (c & 1) * 4);
                f16x8 qh[2], ql[2];
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    const float4 a0 = qraw[2 * ks], a1 = qraw[2 * ks + 1];
                    const float qv[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
                    split_pairs<8>(qv, qh[ks], ql[ks]);
                }
                f32x4 s2t[2];
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const int kt = 2 * wave + t;
                    s2t[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int ks = 0; ks < 2; ++ks) {
                        const int ko = (kt * 16 + fr) * 128 + (((ks * 4 + fq) ^ (lane & 7)) << 4);
                        const f16x8 kh = *reinterpret_cast<const f16x8 *>(Kh + ko);
                        const f16x8 kl = *reinterpret_cast<const f16x8 *>(Kl + ko);
                        s2t[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kh, qh[ks], s2t[t], 0, 0, 0);
                        s2t[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kl, qh[ks], s2t[t], 0, 0, 0);
                        s2t[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kh, ql[ks], s2t[t], 0, 0, 0);
                    }
                }
                float mx = fmaxf(fmaxf(fmaxf(s2t[0][0], s2t[0][1]), fmaxf(s2t[0][2], s2t[0][3])),
                                 fmaxf(fmaxf(s2t[1][0], s2t[1][1]), fmaxf(s2t[1][2], s2t[1][3])));
                mx = xor16_32_max(mx);
                float sx = 0.f;
                if (wave == 0) {   // the extra key (token L-1 as a KEY) belongs to wave 0's share
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const float4 kx = *reinterpret_cast<const float4 *>(Xk + (c >> 1) * 32 + fq * 8 + (c & 1) * 4);
                        sx = fmaf(qraw[c].x, kx.x, sx);
                        sx = fmaf(qraw[c].y, kx.y, sx);
                        sx = fmaf(qraw[c].z, kx.z, sx);
                        sx = fmaf(qraw[c].w, kx.w, sx);
                    }
                    sx = xor16_32_sum(sx);
                    mx = fmaxf(mx, sx);
                }
                const float nmx = fmaf(-mx, scale_log2e, 10.0f);
                float sum = 0.f;
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float pv = __builtin_amdgcn_exp2f(fmaf(s2t[t][r], scale_log2e, nmx));
                        s2t[t][r] = pv;
                        sum += pv;
                    }
                sum = xor16_32_sum(sum);
                float px = 0.f;
                if (wave == 0) {
                    px = __builtin_amdgcn_exp2f(fmaf(sx, scale_log2e, nmx));
                    sum += px;
                }
                f32x4 o[4];
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
                {
                    f16x8 ph, pl;
                    {
                        const float pv[8] = {s2t[0][0], s2t[0][1], s2t[0][2], s2t[0][3], s2t[1][0], s2t[1][1], s2t[1][2], s2t[1][3]};
                        split_pairs<8>(pv, ph, pl);
                    }
#pragma unroll
                    for (int dt = 0; dt < 4; ++dt) {
                        const int trq = fr >> 2, trp = fr & 3;
                        const int row0 = wave * 32 + fq * 4 + trq, row1 = row0 + 16;
                        const int chunk = dt * 2 + (trp >> 1);
                        const int o0 = row0 * 128 + ((chunk ^ (((row0 >> 1) & 3) << 1)) << 4) + (trp & 1) * 8;
                        const int o1 = row1 * 128 + ((chunk ^ (((row1 >> 1) & 3) << 1)) << 4) + (trp & 1) * 8;
                        typedef short s8_t __attribute__((ext_vector_type(8)));
                        const att_s4 h0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((att_lds_s4 *)(Vh + o0));
                        const att_s4 h1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((att_lds_s4 *)(Vh + o1));
                        const att_s4 l0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((att_lds_s4 *)(Vl + o0));
                        const att_s4 l1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((att_lds_s4 *)(Vl + o1));
                        const s8_t vh8 = {h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]};
                        const s8_t vl8 = {l0[0], l0[1], l0[2], l0[3], l1[0], l1[1], l1[2], l1[3]};
                        const f16x8 vh = __builtin_bit_cast(f16x8, vh8), vl = __builtin_bit_cast(f16x8, vl8);
                        o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vh, ph, o[dt], 0, 0, 0);
                        o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vl, ph, o[dt], 0, 0, 0);
                        o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vh, pl, o[dt], 0, 0, 0);
                    }
                }
                if (wave == 0) {
#pragma unroll
                    for (int dt = 0; dt < 4; ++dt) {
                        const float4 vx = *reinterpret_cast<const float4 *>(Xk + 64 + dt * 16 + fq * 4);
                        o[dt][0] = fmaf(px, vx.x, o[dt][0]);
                        o[dt][1] = fmaf(px, vx.y, o[dt][1]);
                        o[dt][2] = fmaf(px, vx.z, o[dt][2]);
                        o[dt][3] = fmaf(px, vx.w, o[dt][3]);
                    }
                }
                // partials of query column 0 (= token L-1; the other fifteen columns are copies): the wave's own patch holds
                // O[64] | max | sum as fp32
                float *pt = reinterpret_cast<float *>(Ot + wave * (16 * OS));
                if (fr == 0) {
#pragma unroll
                    for (int dt = 0; dt < 4; ++dt)
                        *reinterpret_cast<float4 *>(pt + dt * 16 + fq * 4) = make_float4(o[dt][0], o[dt][1], o[dt][2], o[dt][3]);
                    if (fq == 0) {
                        pt[64] = mx;
                        pt[65] = sum;
                    }
                }
                __syncthreads();
                if (wave == 0) {   // merge in wave order (fixed: the result does not depend on timing), lane = output dimension d
                    float mw[NW], lw[NW], M = -3.0e38f;
#pragma unroll
                    for (int w2 = 0; w2 < NW; ++w2) {
                        const float *pw = reinterpret_cast<const float *>(Ot + w2 * (16 * OS));
                        mw[w2] = pw[64];
                        lw[w2] = pw[65];
                        M = fmaxf(M, mw[w2]);
                    }
                    float den = 0.f, num = 0.f;
#pragma unroll
                    for (int w2 = 0; w2 < NW; ++w2) {
                        const float *pw = reinterpret_cast<const float *>(Ot + w2 * (16 * OS));
                        const float sc = __builtin_amdgcn_exp2f((mw[w2] - M) * scale_log2e);
                        den = fmaf(lw[w2], sc, den);
                        num = fmaf(pw[lane], sc, num);
                    }
                    const float v = num / den;
                    const _Float16 hi = (_Float16)v;
                    const _Float16 lo = (_Float16)(v - (float)hi);
                    if (!(dbg & 4)) {
                        _Float16 *orow = out + ((int64_t)b * L + (L - 1)) * 2 * W + h * 64 + lane;
                        orow[0] = hi;
                        orow[W] = lo;
                    }
                }
            }
        }
    }     // (image, head) pairs
}

// ---------------------------------------------------------------------------------------------
// attention for long sequences (256 < L <= MPREID_VIT_MAX_TOKENS), fp16 and split modes: the "key on the lane" scheme of
// the two kernels above, with K / V streamed through LDS in blocks of ATL_KB keys instead of resident for the whole head.
//   grid (B * heads, groups): workgroup (pair, g) owns the query tiles g * tpg .. g * tpg + tpg - 1, one per wave (tpg <= 8;
//   the other waves only stage).  A tile's arithmetic does not depend on g, tpg or the batch: rows are batch-independent.
//   Per key block (two LDS buffers, one barrier per block; block j + 1 is requested into registers before block j is
//   computed and written to the other buffer after it, cdna_hip_programming.md T14):
//     S^T = K Q^T for the block's 16-key tiles, block max over the keys (in-lane + xor 16 / 32)
//     m' = max(m, block max); O^T and the lane's partial row sum *= exp2((m - m') c)   (every block, no deferred max)
//     P^T = exp2(S^T c - m' c) straight from the accumulators into O^T += V^T P^T
//   The rescale precedes the exponentiation of the block's P and follows the previous block's complete P V, so nothing at
//   the old scale is missed and nothing at the new one is scaled twice.
// SPLIT: fp32 q | k | v in, K / V split into hi / lo fp16 pairs while staged, hi.hi' + lo.hi' + hi.lo' for every product and
// P carrying 2^10, exactly the operand scheme of attention_split_kernel; O leaves as the fp16 pair [hi(W) | lo(W)].
// Keys >= L (last block): rows clamped to L - 1 (finite copies), scores forced to -huge, so their P is 0; only the key
// tiles / PV steps that hold a valid key run.
// ---------------------------------------------------------------------------------------------
constexpr int ATL_KB = 64;   // keys per block: four 16-key S^T tiles, two 32-key P V steps
constexpr int ATL_NW = 8;    // waves per workgroup

template <bool SPLIT>
__global__ __launch_bounds__(64 * ATL_NW) void attention_long_kernel(const void *__restrict__ qkv_, int L, int W, int heads,
                                                                     _Float16 *__restrict__ out, int nqt, int tpg) {
    constexpr int NT = 64 * ATL_NW;
    constexpr int ARR = ATL_KB * 128;               // bytes of one [KB][64] fp16 array
    constexpr int BUF = (SPLIT ? 4 : 2) * ARR;      // Kh | Kl | Vh | Vl (split) or K | V (fp16)
    constexpr int NST = SPLIT ? 2 : 1;              // 16-byte staging chunks per thread per array
    static_assert(ATL_KB * (SPLIT ? 16 : 8) == NST * NT, "one block = NST staging chunks per thread");
    static_assert(ATL_NW * 16 * 72 * 2 <= 2 * BUF, "the O patches reuse the two K / V buffers");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    const int pair = blockIdx.x, b = pair / heads, h = pair - b * heads;
    const int64_t ld = 3 * (int64_t)W;
    const int qt = blockIdx.y * tpg + wave;
    const bool active = wave < tpg && qt < nqt;   // wave-uniform
    const int nkb = (L + ATL_KB - 1) / ATL_KB;
    const float scale_log2e = 0.125f * 1.44269504088896340736f;

    typedef typename std::conditional<SPLIT, float, _Float16>::type T;
    const T *base = reinterpret_cast<const T *>(qkv_) + (int64_t)b * L * ld + h * 64;

    // staging registers: (fp16) one 16-byte chunk of K and of V; (split) two chunks of 4 floats of each
    uint4 kr16 = make_uint4(0, 0, 0, 0), vr16 = kr16;
    float4 krf[NST], vrf[NST];
    auto stage_load = [&](int kb) {
        if constexpr (SPLIT) {
#pragma unroll
            for (int i = 0; i < NST; ++i) {
                const int idx = tid + i * NT, row = idx >> 4, c = idx & 15;
                const int key = kb * ATL_KB + row, kc = key < L ? key : L - 1;
                const float *p = reinterpret_cast<const float *>(base) + (int64_t)kc * ld + c * 4;
                krf[i] = load_nt_f4(p + W);
                vrf[i] = load_nt_f4(p + 2 * W);
            }
        } else {
            const int row = tid >> 3, c = tid & 7;
            const int key = kb * ATL_KB + row, kc = key < L ? key : L - 1;
            const _Float16 *p = reinterpret_cast<const _Float16 *>(base) + (int64_t)kc * ld + c * 8;
            kr16 = load_nt16(p + W);
            vr16 = load_nt16(p + 2 * W);
        }
    };
    auto stage_store = [&](int buf) {
        unsigned char *Kb = smem + buf * BUF;
        if constexpr (SPLIT) {
            unsigned char *Kh = Kb, *Kl = Kb + ARR, *Vh = Kb + 2 * ARR, *Vl = Kb + 3 * ARR;
#pragma unroll
            for (int i = 0; i < NST; ++i) {
                const int idx = tid + i * NT, row = idx >> 4, c = idx & 15;
                h4_t hi, lo;
                const int ko = row * 128 + (((c >> 1) ^ (row & 7)) << 4) + (c & 1) * 8;
                split4(krf[i], hi, lo);
                *reinterpret_cast<h4_t *>(Kh + ko) = hi;
                *reinterpret_cast<h4_t *>(Kl + ko) = lo;
                const int vo = row * 128 + (((c >> 1) ^ (((row >> 1) & 3) << 1)) << 4) + (c & 1) * 8;
                split4(vrf[i], hi, lo);
                *reinterpret_cast<h4_t *>(Vh + vo) = hi;
                *reinterpret_cast<h4_t *>(Vl + vo) = lo;
            }
        } else {
            unsigned char *Ks = Kb, *Vs = Kb + ARR;
            const int row = tid >> 3, c = tid & 7;
            *reinterpret_cast<uint4 *>(Ks + row * 128 + ((c ^ (row & 7)) << 4)) = kr16;
            *reinterpret_cast<uint4 *>(Vs + row * 128 + ((c ^ (((row >> 1) & 3) << 1)) << 4)) = vr16;
        }
    };

    // Q of the wave's tile (B operand: B[k = d][col = query], 8 consecutive d per lane per 32-wide k step); rows past L clamped
    f16x8 qh[2], ql[2];
    {
        const int q = (active ? qt : 0) * 16 + fr;
        const int qc = q < L ? q : L - 1;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            if constexpr (SPLIT) {
                const float *qp = reinterpret_cast<const float *>(base) + (int64_t)qc * ld + ks * 32 + fq * 8;
                const float4 a0 = *reinterpret_cast<const float4 *>(qp), a1 = *reinterpret_cast<const float4 *>(qp + 4);
                const float qv[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
                split_pairs<8>(qv, qh[ks], ql[ks]);
            } else {
                qh[ks] = *reinterpret_cast<const f16x8 *>(reinterpret_cast<const _Float16 *>(base) + (int64_t)qc * ld + ks * 32 + fq * 8);
                ql[ks] = qh[ks];
            }
        }
    }

    f32x4 o[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -3.0e38f, lsum = 0.f;   // running max (of the raw scores) of this lane's query column; this lane's partial row sum

    stage_load(0);
    stage_store(0);
    __syncthreads();
    for (int kb = 0; kb < nkb; ++kb) {
        if (kb + 1 < nkb) stage_load(kb + 1);   // in flight while block kb is computed
        if (active) {
            const unsigned char *Kb = smem + (kb & 1) * BUF;
            const unsigned char *Kh = Kb, *Kl = Kb + ARR;
            const unsigned char *Vh = Kb + (SPLIT ? 2 : 1) * ARR, *Vl = Kb + 3 * ARR;
            const int key0 = kb * ATL_KB;
            const int nv = L - key0 < ATL_KB ? L - key0 : ATL_KB;   // valid keys of the block (>= 1)
            const int ntile = (nv + 15) >> 4, nstep = (nv + 31) >> 5;
            f32x4 s[4];
#pragma unroll
            for (int kt = 0; kt < 4; ++kt) {
                s[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (kt < ntile) {
#pragma unroll
                    for (int ks = 0; ks < 2; ++ks) {
                        const int ko = (kt * 16 + fr) * 128 + (((ks * 4 + fq) ^ (lane & 7)) << 4);
                        const f16x8 kh = *reinterpret_cast<const f16x8 *>(Kh + ko);
                        s[kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kh, qh[ks], s[kt], 0, 0, 0);
                        if constexpr (SPLIT) {
                            const f16x8 kl = *reinterpret_cast<const f16x8 *>(Kl + ko);
                            s[kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kl, qh[ks], s[kt], 0, 0, 0);
                            s[kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kh, ql[ks], s[kt], 0, 0, 0);
                        }
                    }
                }
            }
            if (nv < ATL_KB) {   // the last block: keys >= L
#pragma unroll
                for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (kt * 16 + fq * 4 + r >= nv) s[kt][r] = -3.0e38f;
            }
            float bmx = -3.0e38f;
#pragma unroll
            for (int kt = 0; kt < 4; ++kt) bmx = fmaxf(bmx, fmaxf(fmaxf(s[kt][0], s[kt][1]), fmaxf(s[kt][2], s[kt][3])));
            bmx = xor16_32_max(bmx);
            const float mn = fmaxf(m, bmx);
            const float alpha = __builtin_amdgcn_exp2f((m - mn) * scale_log2e);   // 1 when the max did not move; 0 at block 0
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
#pragma unroll
                for (int r = 0; r < 4; ++r) o[dt][r] *= alpha;
            lsum *= alpha;
            m = mn;
            // p = exp2(s c - m c) (split: times 2^10, see attention_split_kernel); masked keys give exp2(-huge) = 0
            const float nmx = SPLIT ? fmaf(-mn, scale_log2e, 10.0f) : -mn * scale_log2e;
#pragma unroll
            for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float p = __builtin_amdgcn_exp2f(fmaf(s[kt][r], scale_log2e, nmx));
                    s[kt][r] = p;
                    lsum += p;
                }
            // O^T += V^T P^T over 32-key steps; P^T fragment element j <-> key 32*s2 + 16*(j>>2) + 4*fq + (j&3)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                if (s2 < nstep) {
                    f16x8 ph, pl;
                    if constexpr (SPLIT) {
                        const float pv[8] = {s[2 * s2][0], s[2 * s2][1], s[2 * s2][2], s[2 * s2][3],
                                             s[2 * s2 + 1][0], s[2 * s2 + 1][1], s[2 * s2 + 1][2], s[2 * s2 + 1][3]};
                        split_pairs<8>(pv, ph, pl);
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            ph[j] = (_Float16)s[2 * s2][j];
                            ph[4 + j] = (_Float16)s[2 * s2 + 1][j];
                        }
                        pl = ph;
                    }
#pragma unroll
                    for (int dt = 0; dt < 4; ++dt) {
                        const int trq = fr >> 2, trp = fr & 3;
                        const int row0 = s2 * 32 + fq * 4 + trq, row1 = row0 + 16;
                        const int chunk = dt * 2 + (trp >> 1);
                        const int o0 = row0 * 128 + ((chunk ^ (((row0 >> 1) & 3) << 1)) << 4) + (trp & 1) * 8;
                        const int o1 = row1 * 128 + ((chunk ^ (((row1 >> 1) & 3) << 1)) << 4) + (trp & 1) * 8;
                        typedef short s8_t __attribute__((ext_vector_type(8)));
                        const att_s4 h0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((att_lds_s4 *)(Vh + o0));
                        const att_s4 h1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((att_lds_s4 *)(Vh + o1));
                        const s8_t vh8 = {h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]};
                        const f16x8 vh = __builtin_bit_cast(f16x8, vh8);
                        o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vh, ph, o[dt], 0, 0, 0);
                        if constexpr (SPLIT) {
                            const att_s4 l0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((att_lds_s4 *)(Vl + o0));
                            const att_s4 l1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((att_lds_s4 *)(Vl + o1));
                            const s8_t vl8 = {l0[0], l0[1], l0[2], l0[3], l1[0], l1[1], l1[2], l1[3]};
                            const f16x8 vl = __builtin_bit_cast(f16x8, vl8);
                            o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vl, ph, o[dt], 0, 0, 0);
                            o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vh, pl, o[dt], 0, 0, 0);
                        }
                    }
                }
            }
        }
        if (kb + 1 < nkb) stage_store((kb + 1) & 1);   // that buffer was last read in block kb - 1, before the barrier below
        __syncthreads();
    }
    // (after the last barrier both K / V buffers are free: they hold the waves' O patches)
    if (!active) return;
    const float sum = xor16_32_sum(lsum);
    const float inv = 1.0f / sum;
    constexpr int OS = 72;
    _Float16 *ot = reinterpret_cast<_Float16 *>(smem) + wave * (16 * OS);
    h4_t ohi[4], olo[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
        const float ovf[4] = {o[dt][0] * inv, o[dt][1] * inv, o[dt][2] * inv, o[dt][3] * inv};
        if constexpr (SPLIT) {
            split_pairs<4>(ovf, ohi[dt], olo[dt]);
        } else {
            ohi[dt] = h4_t{(_Float16)ovf[0], (_Float16)ovf[1], (_Float16)ovf[2], (_Float16)ovf[3]};
            olo[dt] = ohi[dt];
        }
    }
#pragma unroll
    for (int part = 0; part < (SPLIT ? 2 : 1); ++part) {
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
            *reinterpret_cast<h4_t *>(ot + fr * OS + dt * 16 + fq * 4) = part == 0 ? ohi[dt] : olo[dt];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int row = it * 8 + (lane >> 3), ch = lane & 7;
            const uint4 v = *reinterpret_cast<const uint4 *>(ot + row * OS + ch * 8);
            const int qrow = qt * 16 + row;
            if (qrow < L) {
                if constexpr (SPLIT)
                    store_nt16(out + ((int64_t)b * L + qrow) * 2 * W + part * W + h * 64 + ch * 8, v);
                else
                    store_nt16(out + ((int64_t)b * L + qrow) * W + h * 64 + ch * 8, v);
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

template <int KTP, int NW, bool EXACT>
static int launch_attention(const _Float16 *qkv, int B, int L, int W, int heads, _Float16 *out, int q_tiles,
                            hipStream_t stream) {
    constexpr int KEYS = KTP * 16;
    const size_t lds = (size_t)2 * KEYS * 128 + (size_t)NW * 16 * 72 * 2;
    // a process may drive several GPUs (the reference's do_inference is multi-device in one process,
    // processor/processor.py:178-182): the occupancy is queried once per HIP device, after the LDS attribute it depends on
    int dev = 0, cus = 256;
    HIP_TRY(hipGetDevice(&dev));
    int rc = mpreid_dyn_lds(attention_kernel<KTP, NW, EXACT>, lds);
    if (rc) return rc;
    static PerDeviceOnce occ_once;
    static int occ_dev[64] = {};
    int blocks_per_cu = 0;
    rc = occ_once.run([&]() -> int {
        // persistent grid: as many workgroups as fit the chip at once (LDS and the 4-waves/SIMD register
        // bound), each walking pairs with stride gridDim
        int occ = 0;
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(
            &occ, reinterpret_cast<const void *>(attention_kernel<KTP, NW, EXACT>), 64 * NW, lds));
        blocks_per_cu = occ > 0 ? occ : 1;
        if (dev < 64) occ_dev[dev] = blocks_per_cu;
        if (mpreid_tune("verbose", 0))
            fprintf(stderr, "[mpreid] attention<%d,%d,%s> on device %d: %d workgroups/CU by the occupancy API (lds %zu B, %d threads)\n",
                    KTP, NW, EXACT ? "EXACT" : "MASKALL", dev, occ, lds, 64 * NW);
        return MPREID_OK;
    });
    if (rc) return rc;
    if (!blocks_per_cu) blocks_per_cu = occ_dev[dev];   // queried by an earlier call on this device
    if ((rc = mpreid_device_cus(&cus))) return rc;
    const int total = B * heads;
    int grid = cus * blocks_per_cu;
    if (grid > total) grid = total;
    hipLaunchKernelGGL((attention_kernel<KTP, NW, EXACT>), dim3((unsigned)grid), dim3(64 * NW), lds, stream, qkv, L, W,
                       heads, out, q_tiles, total, mpreid_ablation_env("MPREID_ATT_DBG"));
    LAUNCH_CHECK();
    return MPREID_OK;
}

template <int KTP, int NW, bool XKEY = false>
static int launch_attention_split(const float *qkv, int B, int L, int W, int heads, _Float16 *out, int q_tiles,
                                  hipStream_t stream) {
    constexpr int KEYS = KTP * 16;
    const size_t lds = (size_t)4 * KEYS * 128 + (size_t)NW * 16 * 72 * 2 + (XKEY ? 768 : 0);
    int dev = 0, cus = 256;
    HIP_TRY(hipGetDevice(&dev));
    int rc = mpreid_dyn_lds(attention_split_kernel<KTP, NW, XKEY>, lds);
    if (rc) return rc;
    static PerDeviceOnce verbose_once;   // once per instantiation and device, like launch_attention's line
    rc = verbose_once.run([&]() -> int {
        if (mpreid_tune("verbose", 0))
            fprintf(stderr, "[mpreid] attention_split<%d,%d%s> on device %d: lds %zu B, %d threads\n", KTP, NW, XKEY ? ",XKEY" : "",
                    dev, lds, 64 * NW);
        return MPREID_OK;
    });
    if (rc) return rc;
    if ((rc = mpreid_device_cus(&cus))) return rc;
    const int total = B * heads;
    // persistent: as many workgroups as the LDS lets a CU hold (one for L = 129; the small test shapes fit several)
    int per_cu = (int)((160 * 1024) / lds);
    per_cu = per_cu < 1 ? 1 : (per_cu > 4 ? 4 : per_cu);
    int grid = cus * per_cu;
    if (grid > total) grid = total;
    static const int att_dbg = mpreid_ablation_env("MPREID_ATT_DBG");
    hipLaunchKernelGGL((attention_split_kernel<KTP, NW, XKEY>), dim3((unsigned)grid), dim3(64 * NW), lds, stream, qkv, L, W, heads,
                       out, q_tiles, total, att_dbg);
    LAUNCH_CHECK();
    return MPREID_OK;
}

// L > 256: the streaming kernel.  Query tiles are dealt to ceil(tiles / 8) workgroups per (image, head) as evenly as the
// 8 waves allow (L = 257: 17 tiles as 6 + 6 + 5; L = 442: 28 as 7 x 4); a CLS-only call is one workgroup with one tile.
template <bool SPLIT>
static int launch_attention_long(const void *qkv, int B, int L, int W, int heads, _Float16 *out, int q_tiles,
                                 hipStream_t stream) {
    const size_t lds = (size_t)2 * (SPLIT ? 4 : 2) * ATL_KB * 128;
    int rc = mpreid_dyn_lds(attention_long_kernel<SPLIT>, lds);
    if (rc) return rc;
    static PerDeviceOnce verbose_once;
    rc = verbose_once.run([&]() -> int {
        if (mpreid_tune("verbose", 0)) {
            int dev = 0;
            HIP_TRY(hipGetDevice(&dev));
            fprintf(stderr, "[mpreid] attention_long<%s> on device %d: lds %zu B, %d threads\n", SPLIT ? "split" : "fp16", dev, lds,
                    64 * ATL_NW);
        }
        return MPREID_OK;
    });
    if (rc) return rc;
    const int nqt = (q_tiles > 0) ? q_tiles : (L + 15) / 16;
    const int groups = (nqt + ATL_NW - 1) / ATL_NW;
    const int tpg = (nqt + groups - 1) / groups;
    hipLaunchKernelGGL((attention_long_kernel<SPLIT>), dim3((unsigned)(B * heads), (unsigned)groups), dim3(64 * ATL_NW), lds,
                       stream, qkv, L, W, heads, out, nqt, tpg);
    LAUNCH_CHECK();
    return MPREID_OK;
}

int attention_split_dispatch(const float *qkv, int B, int L, int W, int heads, _Float16 *out, int q_tiles, hipStream_t stream) {
    if (L > 256) return launch_attention_long<true>(qkv, B, L, W, heads, out, q_tiles, stream);
    const int kt = (L + 15) / 16;
    if (kt <= 2) return launch_attention_split<2, 2>(qkv, B, L, W, heads, out, q_tiles, stream);
    if (L == 129) return launch_attention_split<8, 4, true>(qkv, B, L, W, heads, out, q_tiles, stream);   // ViT-B/16 at 256 x 128
    if (kt <= 10) return launch_attention_split<10, 8>(qkv, B, L, W, heads, out, q_tiles, stream);
    if (kt <= 14) return launch_attention_split<14, 8>(qkv, B, L, W, heads, out, q_tiles, stream);
    return launch_attention_split<16, 8>(qkv, B, L, W, heads, out, q_tiles, stream);
}

// waves per workgroup: one per 16-query tile when the block can hold them; at least 4 so that the
// K/V staging of a CLS-only call (one query tile) is still spread over 256 threads
int attention_dispatch(const _Float16 *qkv, int B, int L, int W, int heads, _Float16 *out, int q_tiles, hipStream_t stream) {
    if (L > 256) return launch_attention_long<false>(qkv, B, L, W, heads, out, q_tiles, stream);
    const int kt = (L + 15) / 16;
    if (kt <= 2) return launch_attention<2, 2, true>(qkv, B, L, W, heads, out, q_tiles, stream);
    if (kt <= 10) {
        const bool exact = kt >= 9;
        // (L = 129 = nine query tiles: nine waves, one tile each, measured 123 us against 111 for eight waves with wave 0
        // taking tile 8 as well.  Ablations of the 8-wave kernel, same run: loads + LDS staging alone 61 us, compute on
        // stale LDS alone 80 us, stores 5 us)
        // four waves per workgroup (2-3 query tiles each): 50 KB of LDS = three workgroups per CU and no register
        // spills; eight waves (two workgroups per CU under a 128-VGPR bound, 44 B of scratch per lane, wave 0 taking
        // tile 8 as well) measured 113 us against 105 at B = 508, L = 129
        return exact ? launch_attention<10, 4, true>(qkv, B, L, W, heads, out, q_tiles, stream)
                     : launch_attention<10, 4, false>(qkv, B, L, W, heads, out, q_tiles, stream);
    }
    if (kt <= 14)
        return kt >= 13 ? launch_attention<14, 8, true>(qkv, B, L, W, heads, out, q_tiles, stream)
                        : launch_attention<14, 8, false>(qkv, B, L, W, heads, out, q_tiles, stream);
    return launch_attention<16, 8, true>(qkv, B, L, W, heads, out, q_tiles, stream);   // kt is 15 or 16: always EXACT
}

double attention_bytes(int64_t M, int64_t qrows, int W, int pr) {
    return ((double)M * 2.0 * W + (double)qrows * 2.0 * W) * 2.0 * pr;
}

extern "C" int mpreid_vit_attention(const void *qkv, int precision, int B, int L, int W, int heads, int q_tiles, void *out,
                                    mpreid_stream_t stream) {
    ARG_CHECK(qkv && out && B > 0 && heads > 0 && q_tiles >= 0);
    ARG_CHECK(precision == MPREID_VIT_F16 || precision == MPREID_VIT_SPLIT);
    ARG_CHECK(W == 64 * heads && L >= 2 && L <= MPREID_VIT_MAX_TOKENS);
    ARG_CHECK(((uintptr_t)qkv & 15) == 0 && ((uintptr_t)out & 15) == 0);
    if (16 * (int64_t)q_tiles >= L) q_tiles = 0;   // every tile: the kernels' own form of "all rows"
    hipStream_t s = (hipStream_t)stream;
    const int pr = precision == MPREID_VIT_SPLIT ? 2 : 1;
    const int64_t M = (int64_t)B * L;
    const int64_t qrows = q_tiles > 0 ? (int64_t)B * (16 * q_tiles < L ? 16 * q_tiles : L) : M;
    void *ptok = mpreid_prof_begin(s);   // the class of the forward's launches: (MPREID_PROF_ATTENTION, M, q_tiles != 0, pr)
    const int rc = precision == MPREID_VIT_SPLIT
                       ? attention_split_dispatch(reinterpret_cast<const float *>(qkv), B, L, W, heads,
                                                  reinterpret_cast<_Float16 *>(out), q_tiles, s)
                       : attention_dispatch(reinterpret_cast<const _Float16 *>(qkv), B, L, W, heads,
                                            reinterpret_cast<_Float16 *>(out), q_tiles, s);
    mpreid_prof_end(ptok, s, MPREID_PROF_ATTENTION, M, q_tiles ? 1 : 0, pr, attention_bytes(M, qrows, W, pr));
    return rc;
}

// softmax(q k^T / sqrt(64)) v per (image, head), fp32 throughout: K and V of the head in LDS, one thread per query
// row, online softmax.  qkv [B*L][3W] (q | k | v column blocks, head h = columns [64h, 64h + 64)), out [B*L][W].
__global__ __launch_bounds__(256) void attention_f32_kernel(const float *__restrict__ qkv, int L, int W, int heads,
                                                            float *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *Ks = reinterpret_cast<float *>(smem), *Vs = Ks + (size_t)L * 64;
    const int b = blockIdx.x / heads, h = blockIdx.x % heads, tid = threadIdx.x;
    const float *base = qkv + (int64_t)b * L * 3 * W + h * 64;
    for (int idx = tid; idx < L * 16; idx += 256) {
        const int row = idx >> 4, c4 = (idx & 15) * 4;
        *reinterpret_cast<float4 *>(Ks + row * 64 + c4) = *reinterpret_cast<const float4 *>(base + (int64_t)row * 3 * W + W + c4);
        *reinterpret_cast<float4 *>(Vs + row * 64 + c4) = *reinterpret_cast<const float4 *>(base + (int64_t)row * 3 * W + 2 * W + c4);
    }
    __syncthreads();
    for (int t = tid; t < L; t += 256) {
        float q[64], acc[64];
#pragma unroll
        for (int c = 0; c < 64; c += 4) {
            const float4 v = *reinterpret_cast<const float4 *>(base + (int64_t)t * 3 * W + c);
            q[c] = v.x * 0.125f; q[c + 1] = v.y * 0.125f; q[c + 2] = v.z * 0.125f; q[c + 3] = v.w * 0.125f;   // 64^-0.5, exact
            acc[c] = acc[c + 1] = acc[c + 2] = acc[c + 3] = 0.0f;
        }
        float m = -3.402823466e+38f, l = 0.0f;
        for (int j = 0; j < L; ++j) {
            const float *kr = Ks + j * 64, *vr = Vs + j * 64;
            float s = 0.0f;
#pragma unroll
            for (int c = 0; c < 64; ++c) s = fmaf(q[c], kr[c], s);
            const float mn = fmaxf(m, s);
            const float corr = expf(m - mn), pj = expf(s - mn);
            l = l * corr + pj;
#pragma unroll
            for (int c = 0; c < 64; ++c) acc[c] = fmaf(pj, vr[c], acc[c] * corr);
            m = mn;
        }
        float *o = out + ((int64_t)b * L + t) * W + h * 64;
#pragma unroll
        for (int c = 0; c < 64; ++c) o[c] = __fdiv_rn(acc[c], l);
    }
}

// The same per query, for L whose K and V do not fit the LDS at once (L * 512 B > 160 KB, L > 320): K / V pass through LDS in
// chunks of ATF_CHUNK keys.  grid (B * heads, ceil(L / 256)): one query per thread, so a thread's state is one row and every
// thread of the workgroup takes part in the staging; per query the key order and every operation are those of the kernel above.
constexpr int ATF_CHUNK = 128;   // keys per chunk: 64 KB of LDS
__global__ __launch_bounds__(256) void attention_f32_chunked_kernel(const float *__restrict__ qkv, int L, int W, int heads,
                                                                    float *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *Ks = reinterpret_cast<float *>(smem), *Vs = Ks + ATF_CHUNK * 64;
    const int b = blockIdx.x / heads, h = blockIdx.x % heads, tid = threadIdx.x;
    const int t = blockIdx.y * 256 + tid;
    const bool valid = t < L;
    const float *base = qkv + (int64_t)b * L * 3 * W + h * 64;
    float q[64], acc[64];
#pragma unroll
    for (int c = 0; c < 64; c += 4) {
        const float4 v = valid ? *reinterpret_cast<const float4 *>(base + (int64_t)t * 3 * W + c) : make_float4(0.f, 0.f, 0.f, 0.f);
        q[c] = v.x * 0.125f; q[c + 1] = v.y * 0.125f; q[c + 2] = v.z * 0.125f; q[c + 3] = v.w * 0.125f;   // 64^-0.5, exact
        acc[c] = acc[c + 1] = acc[c + 2] = acc[c + 3] = 0.0f;
    }
    float m = -3.402823466e+38f, l = 0.0f;
    for (int j0 = 0; j0 < L; j0 += ATF_CHUNK) {
        const int n = L - j0 < ATF_CHUNK ? L - j0 : ATF_CHUNK;
        __syncthreads();   // every thread is done with the previous chunk
        for (int idx = tid; idx < n * 16; idx += 256) {
            const int row = idx >> 4, c4 = (idx & 15) * 4;
            const float *src = base + (int64_t)(j0 + row) * 3 * W;
            *reinterpret_cast<float4 *>(Ks + row * 64 + c4) = *reinterpret_cast<const float4 *>(src + W + c4);
            *reinterpret_cast<float4 *>(Vs + row * 64 + c4) = *reinterpret_cast<const float4 *>(src + 2 * W + c4);
        }
        __syncthreads();
        if (valid) {
            for (int j = 0; j < n; ++j) {
                const float *kr = Ks + j * 64, *vr = Vs + j * 64;
                float s = 0.0f;
#pragma unroll
                for (int c = 0; c < 64; ++c) s = fmaf(q[c], kr[c], s);
                const float mn = fmaxf(m, s);
                const float corr = expf(m - mn), pj = expf(s - mn);
                l = l * corr + pj;
#pragma unroll
                for (int c = 0; c < 64; ++c) acc[c] = fmaf(pj, vr[c], acc[c] * corr);
                m = mn;
            }
        }
    }
    if (!valid) return;
    float *o = out + ((int64_t)b * L + t) * W + h * 64;
#pragma unroll
    for (int c = 0; c < 64; ++c) o[c] = __fdiv_rn(acc[c], l);
}

// The all-fp32 attention step: K / V of a head resident in LDS where they fit (L * 512 B <= 160 KB, L <= 320), streamed in
// chunks above that.  The one place that takes the choice: the forward's blocks and the unit seam both come through here.
int attention_f32_dispatch(const float *qkv, int B, int L, int W, int heads, float *out, hipStream_t stream) {
    const bool chunked = (size_t)L * 64 * 4 * 2 > 160 * 1024;
    const size_t lds = chunked ? (size_t)ATF_CHUNK * 64 * 4 * 2 : (size_t)L * 64 * 4 * 2;
    const int rc = chunked ? mpreid_dyn_lds(attention_f32_chunked_kernel, lds) : mpreid_dyn_lds(attention_f32_kernel, lds);
    if (rc) return rc;
    if (chunked)
        hipLaunchKernelGGL(attention_f32_chunked_kernel, dim3((unsigned)(B * heads), (unsigned)((L + 255) / 256)), dim3(256), lds,
                           stream, qkv, L, W, heads, out);
    else
        hipLaunchKernelGGL(attention_f32_kernel, dim3((unsigned)(B * heads)), dim3(256), lds, stream, qkv, L, W, heads, out);
    LAUNCH_CHECK();
    return MPREID_OK;
}

extern "C" int mpreid_vit_attention_f32(const float *qkv, int B, int L, int W, int heads, float *out, mpreid_stream_t stream) {
    ARG_CHECK(qkv && out && B > 0 && heads > 0);
    ARG_CHECK(W == 64 * heads && L >= 2 && L <= MPREID_VIT_MAX_TOKENS);
    ARG_CHECK(((uintptr_t)qkv & 15) == 0 && ((uintptr_t)out & 15) == 0);
    return attention_f32_dispatch(qkv, B, L, W, heads, out, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------
// causal attention, split precision: softmax(q k^T / 8 + mask) v per (prompt, head), key j takes part in query row i iff
// j <= i (model/clip/model.py:582-588).  Operands and product terms are attention_split_kernel's: q | k | v fp32 [M][3W],
// K / V split into fp16 pairs while staged into LDS (the layouts of that kernel), Q in registers, every product
// hi.hi' + lo.hi' + hi.lo' into one fp32 accumulator, P carrying 2^10, O leaving as the pair [hi(W) | lo(W)].
// One workgroup per (prompt, head), K / V of the head resident in LDS (L <= 16 * KTP <= MPREID_TEXT_MAX_TOKENS), one
// wave per 16-query tile (wave w owns tile w; KTP waves).  What the mask means here:
//   * masked keys are excluded by SELECTION: their score is replaced by -3e38 before the row maximum, so exp2 gives an
//     exact 0.  No infinity is added anywhere: this file is compiled with -ffinite-math-only (mpreid/build.py).
//   * keys >= L of the last 16-key tile lie above every diagonal of a valid query (j >= L > i): causality alone
//     excludes their scores, there is no separate length mask.
//   * their K / V rows are nevertheless ZERO in LDS (selected while staging; the load address is clamped to row L - 1):
//     a probability of 0 times stale LDS content could be NaN, and the P V steps are 32 keys wide.
//   * key tiles wholly above a query tile's diagonal (kt > qt) are SKIPPED: no Q K products, no exponentials, and no
//     P V step that holds only such tiles (tile qt needs the steps 0 .. qt / 2).  Only the diagonal tile is masked.
//   * a row's bits depend on its own prompt's rows 0 .. i and on nothing else: the workgroup of a (prompt, head) pair
//     reads that pair alone, a tile's arithmetic and its order are fixed by (qt, L), and there is no loop over pairs --
//     the batch, the grid and the scheduling cannot reach a result.
// ---------------------------------------------------------------------------------------------
// The `lo` halves of split_pairs are written by inline assembly (common.h: v_fma_mixlo / mixhi_f16), and a matrix
// instruction that reads a register as an operand needs two wait states after a vector-ALU write of it.  hipcc pads that
// distance for its own instructions and not for a write inside an assembly string, so an MFMA scheduled one instruction
// behind the last v_fma_mixhi_f16 read a stale upper half (seen at KTP = 8: the first P V product of every query tile used
// the old bits in the `lo` of one probability per lane -- 3e-3 slab-relative in the output dimensions 0..15, every other
// dimension exact).  This statement carries the two states and is tied by "+v" behind the split and ahead of the product.
__device__ __forceinline__ void split_lo_settle(f16x8 &lo) { asm volatile("s_nop 1" : "+v"(lo)); }

template <int KTP>
__global__ __launch_bounds__(64 * KTP) void attention_causal_kernel(const float *__restrict__ qkv, int L, int W, int heads,
                                                                    _Float16 *__restrict__ out) {
    static_assert(KTP % 2 == 0 && KTP * 16 <= MPREID_TEXT_MAX_TOKENS, "whole 32-key P V steps, at most the token limit");
    constexpr int NW = KTP, KEYS = KTP * 16, NT = 64 * NW;
    constexpr int K_ITERS = KEYS * 16 / NT;   // 16-byte chunks of a [KEYS][64] fp32 array per thread: 4
    static_assert(K_ITERS * NT == KEYS * 16, "whole staging iterations");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char *Kh = smem, *Kl = smem + KEYS * 128, *Vh = smem + 2 * KEYS * 128, *Vl = smem + 3 * KEYS * 128;
    constexpr int OS = 72;
    _Float16 *Ot = reinterpret_cast<_Float16 *>(smem + 4 * KEYS * 128);   // [NW][16][OS]
    // (the wave index through readfirstlane: the compiler then knows that every `kt <= qt` below is wave-uniform and branches
    // on scalars instead of masking lanes)
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 15, fq = lane >> 4;
    const int64_t ld = 3 * (int64_t)W;
    const int pair = blockIdx.x, b = pair / heads, h = pair - b * heads;
    const float *base = qkv + (int64_t)b * L * ld + h * 64;
    const float scale_log2e = 0.125f * 1.44269504088896340736f;

    // ---- K / V of the head -> fp16 pairs in LDS; rows >= L are zero (loaded from the clamped row L - 1, then replaced) ----
    float4 kr[K_ITERS], vr[K_ITERS];
#pragma unroll
    for (int i = 0; i < K_ITERS; ++i) {
        const int idx = tid + i * NT, row = idx >> 4, c = idx & 15;
        const int rc = row < L ? row : L - 1;
        kr[i] = load_nt_f4(base + (int64_t)rc * ld + W + c * 4);
        vr[i] = load_nt_f4(base + (int64_t)rc * ld + 2 * W + c * 4);
    }
    // Q of the wave's tile (B operand: B[k = d][col = query]); rows >= L are clamped and feed only columns that are not stored
    const int qt = wave;
    const int q = qt * 16 + fr;
    float4 qraw[4];
    {
        const int qc = q < L ? q : L - 1;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const float *qp = base + (int64_t)qc * ld + ks * 32 + fq * 8;
            qraw[2 * ks] = *reinterpret_cast<const float4 *>(qp);
            qraw[2 * ks + 1] = *reinterpret_cast<const float4 *>(qp + 4);
        }
    }
#pragma unroll
    for (int i = 0; i < K_ITERS; ++i) {
        const int idx = tid + i * NT, row = idx >> 4, c = idx & 15;
        const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 kv = row < L ? kr[i] : zero, vv = row < L ? vr[i] : zero;
        h4_t hi, lo;
        const int ko = row * 128 + (((c >> 1) ^ (row & 7)) << 4) + (c & 1) * 8;
        split4(kv, hi, lo);
        *reinterpret_cast<h4_t *>(Kh + ko) = hi;
        *reinterpret_cast<h4_t *>(Kl + ko) = lo;
        const int vo = row * 128 + (((c >> 1) ^ (((row >> 1) & 3) << 1)) << 4) + (c & 1) * 8;
        split4(vv, hi, lo);
        *reinterpret_cast<h4_t *>(Vh + vo) = hi;
        *reinterpret_cast<h4_t *>(Vl + vo) = lo;
    }
    __syncthreads();   // the only workgroup barrier: a wave without a valid query row leaves after it
    if (qt * 16 >= L) return;

    f16x8 qh[2], ql[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        const float4 a0 = qraw[2 * ks], a1 = qraw[2 * ks + 1];
        const float qv[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
        split_pairs<8>(qv, qh[ks], ql[ks]);
        split_lo_settle(ql[ks]);
    }
    // S^T = K Q^T for the key tiles 0 .. qt (wave-uniform bound); C: row = key kt * 16 + fq * 4 + r, column = query q
    f32x4 s[KTP];
#pragma unroll
    for (int kt = 0; kt < KTP; ++kt) {
        s[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (kt <= qt) {
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const int ko = (kt * 16 + fr) * 128 + (((ks * 4 + fq) ^ (lane & 7)) << 4);
                const f16x8 kh = *reinterpret_cast<const f16x8 *>(Kh + ko);
                const f16x8 kl = *reinterpret_cast<const f16x8 *>(Kl + ko);
                s[kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kh, qh[ks], s[kt], 0, 0, 0);
                s[kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kl, qh[ks], s[kt], 0, 0, 0);
                s[kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kh, ql[ks], s[kt], 0, 0, 0);
            }
        }
    }
    // the mask, by selection: key > query.  Below the diagonal tile nothing is masked (key < 16 qt <= q); key 0 <= q is
    // never masked, so the maximum is a real score
    float mx = -3.0e38f;
#pragma unroll
    for (int kt = 0; kt < KTP; ++kt) {
        if (kt <= qt) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (kt * 16 + fq * 4 + r > q) s[kt][r] = -3.0e38f;
            mx = fmaxf(mx, fmaxf(fmaxf(s[kt][0], s[kt][1]), fmaxf(s[kt][2], s[kt][3])));
        }
    }
    mx = xor16_32_max(mx);
    // p * 2^10 = exp2(s*c - mx*c + 10); masked entries give exp2(-huge) = 0, skipped tiles are 0 without an exponential
    const float nmx = fmaf(-mx, scale_log2e, 10.0f);
    float sum = 0.f;
#pragma unroll
    for (int kt = 0; kt < KTP; ++kt) {
        if (kt <= qt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = __builtin_amdgcn_exp2f(fmaf(s[kt][r], scale_log2e, nmx));
                s[kt][r] = p;
                sum += p;
            }
        }
    }
    sum = xor16_32_sum(sum);
    // O^T = V^T P^T over the 32-key steps that hold a computed tile; the upper half of step qt / 2 is tile qt + 1 when qt is
    // even: P = 0 there and its V rows are the prompt's own finite rows or the zero rows >= L
    f32x4 o[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s2 = 0; s2 < KTP / 2; ++s2) {
        if (2 * s2 <= qt) {
            f16x8 ph, pl;
            {
                const float pv[8] = {s[2 * s2][0], s[2 * s2][1], s[2 * s2][2], s[2 * s2][3],
                                     s[2 * s2 + 1][0], s[2 * s2 + 1][1], s[2 * s2 + 1][2], s[2 * s2 + 1][3]};
                split_pairs<8>(pv, ph, pl);
                split_lo_settle(pl);
            }
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                const int trq = fr >> 2, trp = fr & 3;
                const int row0 = s2 * 32 + fq * 4 + trq, row1 = row0 + 16;
                const int chunk = dt * 2 + (trp >> 1);
                const int o0 = row0 * 128 + ((chunk ^ (((row0 >> 1) & 3) << 1)) << 4) + (trp & 1) * 8;
                const int o1 = row1 * 128 + ((chunk ^ (((row1 >> 1) & 3) << 1)) << 4) + (trp & 1) * 8;
                typedef short s8_t __attribute__((ext_vector_type(8)));
                const att_s4 h0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((att_lds_s4 *)(Vh + o0));
                const att_s4 h1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((att_lds_s4 *)(Vh + o1));
                const att_s4 l0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((att_lds_s4 *)(Vl + o0));
                const att_s4 l1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((att_lds_s4 *)(Vl + o1));
                const s8_t vh8 = {h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]};
                const s8_t vl8 = {l0[0], l0[1], l0[2], l0[3], l1[0], l1[1], l1[2], l1[3]};
                const f16x8 vh = __builtin_bit_cast(f16x8, vh8), vl = __builtin_bit_cast(f16x8, vl8);
                o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vh, ph, o[dt], 0, 0, 0);
                o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vl, ph, o[dt], 0, 0, 0);
                o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vh, pl, o[dt], 0, 0, 0);
            }
        }
    }
    // O^T -> fp16 pair, through the wave's LDS patch as whole 128-byte rows: hi part, then lo part (attention_split_kernel)
    const float inv = 1.0f / sum;
    _Float16 *ot = Ot + wave * (16 * OS);
    h4_t ohi[4], olo[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
        const float ovf[4] = {o[dt][0] * inv, o[dt][1] * inv, o[dt][2] * inv, o[dt][3] * inv};
        split_pairs<4>(ovf, ohi[dt], olo[dt]);
    }
#pragma unroll
    for (int part = 0; part < 2; ++part) {
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
            *reinterpret_cast<h4_t *>(ot + fr * OS + dt * 16 + fq * 4) = part == 0 ? ohi[dt] : olo[dt];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int row = it * 8 + (lane >> 3), ch = lane & 7;
            const uint4 v = *reinterpret_cast<const uint4 *>(ot + row * OS + ch * 8);
            const int qrow = qt * 16 + row;
            if (qrow < L) store_nt16(out + ((int64_t)b * L + qrow) * 2 * W + part * W + h * 64 + ch * 8, v);
        }
        __builtin_amdgcn_wave_barrier();
    }
}

template <int KTP>
static int launch_attention_causal(const float *qkv, int B, int L, int W, int heads, _Float16 *out, hipStream_t stream) {
    constexpr int KEYS = KTP * 16;
    const size_t lds = (size_t)4 * KEYS * 128 + (size_t)KTP * 16 * 72 * 2;
    int rc = mpreid_dyn_lds(attention_causal_kernel<KTP>, lds);
    if (rc) return rc;
    static PerDeviceOnce verbose_once;
    rc = verbose_once.run([&]() -> int {
        if (mpreid_tune("verbose", 0)) {
            int dev = 0;
            HIP_TRY(hipGetDevice(&dev));
            fprintf(stderr, "[mpreid] attention_causal<%d> on device %d: lds %zu B, %d threads\n", KTP, dev, lds, 64 * KTP);
        }
        return MPREID_OK;
    });
    if (rc) return rc;
    hipLaunchKernelGGL((attention_causal_kernel<KTP>), dim3((unsigned)(B * heads)), dim3(64 * KTP), lds, stream, qkv, L, W, heads,
                       out);
    LAUNCH_CHECK();
    return MPREID_OK;
}

// one wave per 16-query tile and K / V for the even round-up of the key tiles (the P V steps are 32 keys wide)
int attention_causal_dispatch(const float *qkv, int B, int L, int W, int heads, _Float16 *out, hipStream_t stream) {
    const int kt = (L + 15) / 16;
    if (kt <= 2) return launch_attention_causal<2>(qkv, B, L, W, heads, out, stream);
    if (kt <= 4) return launch_attention_causal<4>(qkv, B, L, W, heads, out, stream);
    if (kt <= 6) return launch_attention_causal<6>(qkv, B, L, W, heads, out, stream);   // CLIP's 77 tokens
    return launch_attention_causal<8>(qkv, B, L, W, heads, out, stream);
}

static int text_attention_profiled(const float *qkv, int B, int L, int W, int heads, _Float16 *out, hipStream_t s) {
    // filed like the encoder's launches (vit.hip attention_profiled): (MPREID_PROF_ATTENTION, M, every row, pairs)
    const int64_t M = (int64_t)B * L;
    void *ptok = mpreid_prof_begin(s);
    const int rc = attention_causal_dispatch(qkv, B, L, W, heads, out, s);
    mpreid_prof_end(ptok, s, MPREID_PROF_ATTENTION, M, 0, 2, attention_bytes(M, M, W, 2));
    return rc;
}

extern "C" int mpreid_text_attention(const void *qkv, int B, int L, int W, int heads, void *out, mpreid_stream_t stream) {
    ARG_CHECK(qkv && out && B > 0);
    ARG_CHECK(((uintptr_t)qkv & 15) == 0 && ((uintptr_t)out & 15) == 0);
    const int rc = text_check_shape(L, W, heads);
    if (rc) return rc;
    ARG_CHECK((int64_t)B * heads < (int64_t)1 << 31 && (int64_t)B * L * 3 * W < (int64_t)1 << 40);
    return text_attention_profiled(reinterpret_cast<const float *>(qkv), B, L, W, heads, reinterpret_cast<_Float16 *>(out),
                                   (hipStream_t)stream);
}
