// experts_gemm_plan of tmac_amd/csrc/tmac_launch_plan.cpp as a stand-alone program (tests/test_experts_gemm_cpu.py): one query per line of
// stdin, "plan K bits gs ags nbanks Mw0 Mw1 N S E P"; one answer per line of stdout: "gx gy wg_end0 wg_end1 lds_bytes" or "refuse: <why>".
#include <stdio.h>

#include "../../tmac_amd/csrc/tmac_launch_plan.h"

using namespace tmac;

int main() {
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        int K, bits, gs, ags, nb, mw[2];
        long long n, sl, e, pp;
        if (sscanf(line, "plan %d %d %d %d %d %d %d %lld %lld %lld %lld", &K, &bits, &gs, &ags, &nb, &mw[0], &mw[1], &n, &sl, &e, &pp) != 11) { printf("?\n"); continue; }
        Shape s{};
        s.K = K; s.bits = bits; s.gs = gs; s.ags = ags; s.m_groups = -1; s.zero_point = 1; s.ts = 8; s.lay = 2;
        ExpertsGemmPlan p;
        if (!experts_gemm_plan(s, mw, nb, n, sl, e, pp, p)) printf("refuse: %s\n", p.why);
        else printf("%d %d %d %d %zu\n", p.gx, p.gy, p.wg_end[0], p.wg_end[1], p.lds_bytes);
    }
    return 0;
}
