// The fp16 GEMM launcher's plan (mp-reid_amd/csrc/gemm_plan.h) as a host program: tests/test_gemm_plan_cpu.py compiles this
// file for the host only and runs it.  No HIP runtime call, no device.
//   gemm_plan_main plan   reads lines "epi M N K kseg sym same_operand has_out cus tune-string" ("-": no tuning string; the
//                         program adds verbose=1) and prints the plan's verbose line, or "ERROR <message>"
//   gemm_plan_main dbg    (built with -DMPREID_ABLATION) reads lines "epi dbg" and prints "epi dbg D stamps": the instance
//                         gemm_f16_big_kernel<epi, D> that MPREID_GEMM_DBG=dbg selects and whether it takes the stamps buffer;
//                         epi -1 stands for dist_sym_p2_kernel<D> and MPREID_TUNE=dist_sym_p2_abl
#include <cstring>
#include <string>
#include <utility>

#include "../mp-reid_amd/csrc/gemm_plan.h"

// MPREID_TUNE's grammar (api.cpp): key=value items separated by commas, a bare key means 1
static int tune_of(const std::string &s, const char *key, int dflt) {
    size_t pos = 0;
    while (pos <= s.size()) {
        size_t end = s.find(',', pos);
        if (end == std::string::npos) end = s.size();
        const std::string item = s.substr(pos, end - pos);
        pos = end + 1;
        const size_t eq = item.find('=');
        if (item.substr(0, eq) == key) return eq == std::string::npos ? 1 : atoi(item.c_str() + eq + 1);
    }
    return dflt;
}

static int plan_lines() {
    static _Float16 op_a[1], op_w[1];
    static float out[1];
    int epi, M, N, K, kseg, sym, same, has_out, cus;
    char tune[256];
    while (scanf("%d %d %d %d %d %d %d %d %d %255s", &epi, &M, &N, &K, &kseg, &sym, &same, &has_out, &cus, tune) == 10) {
        const std::string ts = (strcmp(tune, "-") ? std::string(tune) + "," : std::string()) + "verbose=1";
        const GemmTune t = gemm_tune_read([&](const char *key, int dflt) { return tune_of(ts, key, dflt); });
        GemmArgs a{};
        a.A = op_a;
        a.W = same ? op_a : op_w;
        a.M = M; a.N = N; a.K = K; a.kseg = kseg;
        a.sym = sym;
        a.out = has_out ? out : nullptr;
        const GemmPlan p = plan_gemm(epi, a, cus, t);
        printf("%s%s\n", p.status ? "ERROR " : "", p.text);
    }
    return 0;
}

#ifdef MPREID_ABLATION
struct Picked {
    int d, stamps;
};
template <int... EPI>
static Picked picked_of(int epi, int dbg, std::integer_sequence<int, EPI...>) {
    Picked r{-1, 0};
    const auto pick = [](auto d) { return Picked{decltype(d)::value, gemm_dbg_takes_stamps(decltype(d)::value) ? 1 : 0}; };
    ((epi == EPI ? (void)(r = gemm_dbg_select<GEMM_DBG_LIST<EPI>>(dbg, pick)) : (void)0), ...);
    if (epi == -1) r = Picked{gemm_dbg_select<P2_ABL_LIST>(dbg, pick).d, 0};   // (that kernel takes the buffer whenever one is given)
    return r;
}
static int dbg_lines() {
    int epi, dbg;
    while (scanf("%d %d", &epi, &dbg) == 2) {
        const Picked r = picked_of(epi, dbg, std::make_integer_sequence<int, GE_S_BIAS_RES_PAIR + 1>{});
        printf("%d %d %d %d\n", epi, dbg, r.d, r.stamps);
    }
    return 0;
}
#endif

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "plan")) return plan_lines();
#ifdef MPREID_ABLATION
    if (argc == 2 && !strcmp(argv[1], "dbg")) return dbg_lines();
#endif
    fprintf(stderr, "usage: gemm_plan_main plan|dbg < lines\n");
    return 2;
}
