// Stand-alone driver of the GEMM launch plan (nobs-whisper_amd/csrc/gemm_plan.h) for tests/test_gemm_plan.py:
// no GPU, no HIP.
//
//   g++ -std=c++17 -O1 -g [-fsanitize=address,undefined] -I nobs-whisper_amd/csrc tools/gemm_plan_check.cpp
//       nobs-whisper_amd/csrc/gemm_plan.cpp -o gemm_plan_check && ./gemm_plan_check < cases
//
// Input, one call per line: "epi M N K has_ws ws_elems fused_ln w8 variant dec_splits dec_bm gm_env [partials]"
// (partials = 1: the plan of launch_gemm_partials; 0 when left out).
// Output, one line per call:
//   "error <text>"                    the call fails with this text
//   "none"                            partials only: no slabs for this shape / workspace (the launcher returns 0)
//   "kernel bm bn grid_x grid_y grid_z threads tiles_n split splits kc gm reduce red_grid red_threads red_npt"
//                                     kernel 8p | glds | dec | reg, reduce none | plain | ln | ln4
#include <cstdio>

#include "gemm_plan.h"

using namespace wm;

int main() {
    static const char* const kname[] = {"8p", "glds", "dec", "reg"};
    static const char* const rname[] = {"none", "plain", "ln", "ln4"};
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        GemmShape s{};
        GemmKnobs k;
        int has_ws, fused_ln, w8, partials = 0;
        const int n = sscanf(line, "%d %d %d %d %d %ld %d %d %d %d %d %d %d", &s.epi, &s.M, &s.N, &s.K, &has_ws, &s.ws_elems,
                             &fused_ln, &w8, &k.variant, &k.dec_splits, &k.dec_bm_min, &k.group_m_env, &partials);
        if (n < 12) return 2;
        s.has_ws = has_ws != 0; s.fused_ln = fused_ln != 0; s.w8 = w8 != 0; s.partials = partials != 0;
        const GemmPlan p = gemm_plan(s, k);
        if (p.error[0]) printf("error %s\n", p.error);
        else if (s.partials && !p.splits) printf("none\n");
        else
            printf("%s %d %d %d %d %d %d %d %d %d %d %d %s %d %d %d\n", kname[p.kernel], p.bm, p.bn, p.grid_x, p.grid_y, p.grid_z,
                   p.threads, p.tiles_n, (int)p.split, p.splits, p.kc, p.gm, rname[p.reduce], p.red_grid, p.red_threads, p.red_npt);
    }
    return 0;
}
