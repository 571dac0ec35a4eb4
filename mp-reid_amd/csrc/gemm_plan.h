// gemm_plan.h — what launch_gemm_f16 decides before it launches: which of the three fp16 GEMM kernels runs a problem, on
// which grid, and what MPREID_TUNE=verbose=1 says about it.  plan_gemm is a pure function of (epilogue, GemmArgs, CU count,
// tuning switches): no HIP call, no getenv, no error state, so tests/test_gemm_plan_cpu.py compiles it for the host and checks
// its decisions without a GPU.  launch_one (gemm_f16.hip) turns a plan into one launch.
#pragma once
#include <algorithm>
#include <type_traits>

#include "gemm_f16.h"

// The launcher's MPREID_TUNE keys (include/mpreid.h says what each value selects), read once per process: gemm_tune, gemm_f16.hip
struct GemmTune {
    int gemm_big, dist_sym_p2, dist_p2_full, dist_sym_p2_naps, dist_sym_p2_grid, dist_sym_p2_strip, gemm_stagger_all, gemm_walk,
        gemm_ragged, gemm_grid, verbose;
};
template <typename F>   // F: int(const char *key, int dflt) -- mpreid_tune in the library
GemmTune gemm_tune_read(F tune) {
    return {tune("gemm_big", 1), tune("dist_sym_p2", 1), tune("dist_p2_full", 0), tune("dist_sym_p2_naps", -1),
            tune("dist_sym_p2_grid", 0), std::max(1, tune("dist_sym_p2_strip", 8)), tune("gemm_stagger_all", 0), tune("gemm_walk", -1),
            tune("gemm_ragged", 1), tune("gemm_grid", 0), tune("verbose", 0)};
}

enum GemmForm {
    GF_128,       // gemm_f16_kernel: 128x128 tiles, one workgroup per tile
    GF_BIG,       // gemm_f16_big_kernel: persistent 256x256, one workgroup per CU
    GF_BIG_SYM,   // ... its GE_EUCLID instance with the mirrored stores (a symmetric problem)
    GF_P2_SYM,    // dist_sym_p2_kernel: two workgroups per CU, 256x128, a symmetric problem
    GF_P2_FULL    // ... two tensors
};
struct GemmPlan {
    int status;               // MPREID_OK, or MPREID_ERR_ARG: then `text` is the message for mpreid_set_error("%s", ...)
    char text[160];           // else the MPREID_TUNE=verbose=1 line (without the "[mpreid] " prefix; empty without verbose)
    GemmForm form;
    int tiles_m, tiles_n;     // of the form's tile
    unsigned grid, block;
    size_t lds;               // dynamic LDS bytes
    int walk, stagger, stagger_mode;   // GemmArgs fields the launcher writes into its copy of the arguments
    int naps, strip;          // GF_P2_*: the kernel's last two arguments
};

// The tile walk gemm_f16_big_kernel takes, for the verbose line: a COPY of the kernel's three expressions GR / owned / blocked (nb = grid
// size, walk = GemmArgs::walk, sym = a symmetric problem on an epilogue that knows them; neither mode = the plain strided walk).
// A copy, not a function the kernel shares: routed through one, every instantiation of the kernel compiled to a different scalar
// prologue and register assignment.  Whoever changes the kernel's rule changes this one with it; the walk names the tests expect
// (tests/test_gpu_rn50_split_layers.py) are written down by hand and would disagree with a stale copy's.
struct BigWalk { int GR; bool owned, blocked; };
inline BigWalk big_walk_of(int tiles_m, int tiles_n, int nb, int walk, bool sym) {
    BigWalk w;
    w.GR = ((walk & 7) == 3 || (walk & 8)) ? 4 : ((walk & 7) == 4 ? 16 : 8);
    const int ngroups = (tiles_m + w.GR - 1) / w.GR;
    w.owned = (nb % 8 == 0) && (tiles_m % (8 * w.GR) == 0 || (ngroups >= 24 && !(walk & 16) && !sym));
    w.blocked = !w.owned && (nb % 64 == 0) && tiles_m * tiles_n >= nb;
    return w;
}

// a.M, a.N, a.K: positive multiples of GBM / GBN / GBK (launch_gemm_f16 has checked); cus: CU count of the device
inline GemmPlan plan_gemm(int epi, const GemmArgs &a, int cus, const GemmTune &t) {
    GemmPlan p{};
    p.walk = a.walk;
    p.stagger = a.stagger;
    p.stagger_mode = a.stagger_mode;
    p.status = MPREID_ERR_ARG;
    if (gemm_epi_is_split(epi) && (a.kseg <= 0 || a.kseg % GBK || a.K != 2 * a.kseg)) {
        snprintf(p.text, sizeof p.text, "gemm_f16: split epilogue %d needs K == 2 * kseg, kseg a multiple of %d (K=%d kseg=%d)", epi, GBK,
                 a.K, a.kseg);
        return p;
    }
    if (epi == GE_CAND && (a.M % BBM || a.N % BBN)) {
        snprintf(p.text, sizeof p.text, "gemm_f16: the candidate epilogue needs M, N multiples of %d", BBM);
        return p;
    }
    p.status = MPREID_OK;
    const auto shape = [&](GemmForm form, int bm, int bn, unsigned block, size_t lds) {
        p.form = form;
        p.tiles_m = a.M / bm;
        p.tiles_n = a.N / bn;
        p.block = block;
        p.lds = lds;
    };
    const bool use_big = gemm_epi_has_big(epi) &&
                         (epi == GE_CAND || (t.gemm_big > 0 && (a.M % BBM == 0) && (a.N % BBN == 0) &&
                                             (t.gemm_big >= 2 || (int64_t)(a.M / BBM) * (a.N / BBN) >= 128)));
    // two workgroups per CU (before the persistent form).  dist_sym_p2: symmetric stored distance problems of at least 16 tile
    // rows (1, default), whenever the padded size allows (2, tests), also the 3-term split operands, A != W (3: measured slower,
    // see DESIGN).  dist_p2_full: TWO tensors, never (0, default: measured slower), from 16 x 32 tiles
    // (1), whenever the padded sizes allow (2, tests)
    bool use_p2 = false, p2_full = false;
    if (epi == GE_EUCLID) {
        use_p2 = a.sym && t.dist_sym_p2 > 0 && a.M == a.N && (a.A == a.W || t.dist_sym_p2 >= 3) && (a.M % PBM == 0) &&
                 (a.K % PBK == 0) && (t.dist_sym_p2 >= 2 || a.M / PBM >= 16);
        if (!use_p2 && !a.sym && t.dist_p2_full > 0 && a.out && (a.M % PBM == 0) && (a.N % PBN == 0) && (a.K % PBK == 0) &&
            (t.dist_p2_full >= 2 || (a.M / PBM >= 16 && a.N / PBN >= 32)))
            use_p2 = p2_full = true;
    }
    if (use_p2) {
        shape(p2_full ? GF_P2_FULL : GF_P2_SYM, PBM, PBN, 256, P_LDS_BYTES);
        p.grid = (unsigned)(t.dist_sym_p2_grid ? t.dist_sym_p2_grid : std::max(8, (2 * cus) & ~7));
        p.naps = t.dist_sym_p2_naps >= 0 ? t.dist_sym_p2_naps : 0;   // (experiments) late start of every CU's second workgroup, units of s_sleep 8
        p.strip = t.dist_sym_p2_strip;                               // tile rows per strip of the walk
        if (t.verbose)
            snprintf(p.text, sizeof p.text, "gemm epi %d: two workgroups per CU 256x128%s, %dx%d tiles, grid %u", epi,
                     p2_full ? " (two tensors)" : " (symmetric)", p.tiles_m, p.tiles_n, p.grid);
    } else if (use_big) {
        // persistent: one workgroup per CU (the kernel owns the CU's whole LDS), each walking tiles
        shape(epi == GE_EUCLID && a.sym ? GF_BIG_SYM : GF_BIG, BBM, BBN, 512, B_LDS_TOTAL);
        if (t.gemm_stagger_all > 0) {
            p.stagger = t.gemm_stagger_all;
            p.stagger_mode = 1;
        }
        // tile order inside an XCD's row group (bit-identical results; measured: tools/walk_ab.sh, docs/HISTORY_r06.md "Tile
        // order"): auto (-1) = column-fastest for narrow outputs with operand rows of >= 8 KB, i.e. the split FC2 (-2.4 %)
        p.walk = t.gemm_walk >= 3 ? t.gemm_walk
               : (t.gemm_walk == 2 || (t.gemm_walk == 1 && p.tiles_n <= 4) || (t.gemm_walk < 0 && p.tiles_n <= 4 && (int64_t)a.K * 2 >= 8192)) ? 1 : 0;
        // row groups of 4 tile rows when groups of 8 do not divide among the XCDs but groups of 4 do (e.g. tiles_m = 224):
        // bit 3 of walk
        if (t.gemm_walk < 3 && p.tiles_m % 64 != 0 && p.tiles_m % 32 == 0) p.walk |= 8;
        if (!t.gemm_ragged) p.walk |= 16;   // round 5's rule (owned walk only for exact divisions)
        const unsigned total_tiles = (unsigned)p.tiles_m * (unsigned)p.tiles_n;
        if (t.gemm_grid > 0 && t.gemm_grid < cus) cus = t.gemm_grid;   // experiment: persistent workgroups on fewer CUs (same bits)
        p.grid = total_tiles < (unsigned)cus ? total_tiles : (unsigned)cus;
        if (t.verbose) {   // (the walk: big_walk_of, the copy of the kernel's rule)
            const bool sym = (epi == GE_CAND || epi == GE_EUCLID) && a.sym;
            const BigWalk bw = big_walk_of(p.tiles_m, p.tiles_n, (int)p.grid, p.walk, sym);
            char wname[64];
            if (bw.owned)
                snprintf(wname, sizeof wname, "%sowned GR=%d %s", p.tiles_m % (8 * bw.GR) ? "ragged-" : "", bw.GR,
                         (p.walk & 7) == 1 ? "column-fastest" : "row-fastest");
            else
                snprintf(wname, sizeof wname, "%s", bw.blocked ? (sym ? "blocked compacted" : "blocked") : "strided");
            // (the stored-distance epilogue's symmetric instance -- mirrored stores -- says so: the walk name alone does not)
            snprintf(p.text, sizeof p.text, "gemm epi %d: persistent 256x256%s, walk %s, %dx%d tiles, grid %u", epi,
                     p.form == GF_BIG_SYM ? " (symmetric)" : "", wname, p.tiles_m, p.tiles_n, p.grid);
        }
    } else {
        shape(GF_128, GBM, GBN, 256, G_LDS_BYTES);
        p.grid = (unsigned)p.tiles_m * (unsigned)p.tiles_n;
        if (t.verbose) snprintf(p.text, sizeof p.text, "gemm epi %d: 128x128, %dx%d tiles, grid %u", epi, p.tiles_m, p.tiles_n, p.grid);
    }
    return p;
}

#ifdef MPREID_ABLATION
// Timing-ablation instances (WRONG RESULTS by design; common.h), selected by MPREID_GEMM_DBG / MPREID_TUNE=dist_sym_p2_abl: the DBG
// values gemm_f16_big_kernel<EPI, DBG> is instantiated for, per epilogue, and the abl values of dist_sym_p2_kernel<abl>.  Any
// other value runs the plain instance.  64 (split epilogues): operand panels aliased onto two (L2-resident), see set_tile;
// 32: per-tile phase stamps (tools/gemm_tile_stamps.py), 800: stamps + raw stores -- both take GemmArgs::stamps from
// MPREID_GEMM_STAMPS; GE_BIAS_F16: the k-loop ablations (1 no DMA, 2 no MFMA, 4 no fragment reads, 8 no epilogue, 16 the
// unpaired DMA schedule); GE_EUCLID / GE_BIAS_GELU: F * 128, F = 1..6, store cache policies, 16 the unpaired DMA schedule
struct GemmDbgList { int n, v[12]; };
constexpr GemmDbgList gemm_dbg_list(int epi) {
    if (!gemm_epi_has_big(epi)) return {0, {}};
    if (gemm_epi_is_split(epi)) return {2, {64, 32}};
    if (epi == GE_BIAS_F16) return {12, {32, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 24}};
    if (epi == GE_EUCLID || epi == GE_BIAS_GELU) return {9, {800, 32, 1 * 128, 2 * 128, 3 * 128, 4 * 128, 5 * 128, 6 * 128, 16}};
    return {1, {32}};
}
template <int EPI>
inline constexpr GemmDbgList GEMM_DBG_LIST = gemm_dbg_list(EPI);
constexpr GemmDbgList P2_ABL_LIST = {10, {1, 2, 3, 4, 8, 9, 16, 24, 32, 33}};
constexpr bool gemm_dbg_takes_stamps(int dbg) { return dbg == 32 || dbg == 800; }
// f(std::integral_constant<int, D>) for the entry D of the list that equals `dbg`, else for D = 0
template <const GemmDbgList &L, int I = 0, typename F>
auto gemm_dbg_select(int dbg, F f) {
    if constexpr (I < L.n) return dbg == L.v[I] ? f(std::integral_constant<int, L.v[I]>{}) : gemm_dbg_select<L, I + 1>(dbg, f);
    else return f(std::integral_constant<int, 0>{});
}
#endif
