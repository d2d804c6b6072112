// The bias planner of tmac_amd/csrc/tmac_launch_plan.cpp (quad_plan_bias) as a stand-alone program (tests/test_bias_cpu.py): one query per
// line of stdin, one answer per line of stdout -- the plan's fields, or "refuse".  Behind a plan: "| inst 0|1", the policy predicate of the
// bias instantiation it names (quad_bi_inst_exists), and "| twin" + the same fields of the plan the call without a bias gets
// (quad_plan_perm's rule for a built LUT, quad_plan's for a copied one; quad_plan_xf's with a transform), or "| twin refuse".
//   b bits K sm total_q build_lut xf_kind force_ft force_wpq strict      (sm 0: per-group scales, 2: unified scale)
#include <stdio.h>

#include "../../tmac_amd/csrc/tmac_launch_plan.h"

using namespace tmac;

static Shape shape(int bits, int K, int sm) {
    Shape s{};
    s.Mw = 4096; s.K = K; s.bits = bits; s.ts = 8; s.lay = 2;
    if (sm == 2) { s.gs = 0; s.ags = K; s.m_groups = 1; } else { s.gs = 64; s.ags = 64; s.m_groups = -1; }
    return s;
}

static void print_fields(const QuadPlan& p) {
    printf("%d %d %d %d %d %d %d %d %d %d %d %zu", p.ft, p.wpq, p.nr, (int)p.early, (int)p.dump, p.acc, p.lutsrc, (int)p.xf, (int)p.gn, (int)p.gt, p.gx,
           p.lds_bytes);
}

int main() {
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        int bits, K, sm, tq, bl, kind, ft, wq, strict;
        if (sscanf(line, "b %d %d %d %d %d %d %d %d %d", &bits, &K, &sm, &tq, &bl, &kind, &ft, &wq, &strict) != 9) { printf("?\n"); continue; }
        const Shape s = shape(bits, K, sm);
        QuadPlan p, t;
        if (!quad_plan_bias(s, tq, bl != 0, kind, ft, wq, strict != 0, p)) { printf("refuse\n"); continue; }
        print_fields(p);
        printf(" | bi %d ga %d | inst %d", (int)p.bi, (int)p.ga, (int)quad_bi_inst_exists(p.lutsrc, p.nr, p.ft, p.wpq, p.early, p.xf));
        const bool ok = kind ? quad_plan_xf(s, tq, kind, ft, wq, strict != 0, t) : bl ? quad_plan_perm(s, tq, ft, wq, strict != 0, t) : quad_plan(s, tq, false, false, true, ft, wq, t);
        printf(" | twin ");
        if (ok) print_fields(t); else printf("refuse");
        printf("\n");
    }
    return 0;
}
