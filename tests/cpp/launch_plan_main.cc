// The launch planners of tmac_amd/csrc/tmac_launch_plan.cpp as a stand-alone program (tests/test_launch_plan_cpu.py): one query per line of
// stdin, one answer per line of stdout -- every field of the plan, or "refuse".  Behind a plan: "| inst 0|1", the policy predicate of the
// instantiation it names.
//   q bits K sm total_q build_lut dump acc_mfma force_ft force_wpq   k_gemv_quad         (sm 0: per-group scales, 2: unified scale)
//   x bits K sm total_q xf_kind force_ft force_wpq strict            k_gemv_quad, XF
//   r K N total_q                                                    k_gemv_rows: the row groups, waves per quad and launches
//   p K N                                                            rows_plan alone (tmac_hip_debug_rows_plan)
#include <stdio.h>

#include "../../tmac_amd/csrc/tmac_launch_plan.h"

using namespace tmac;

static Shape shape(int bits, int K, int sm) {
    Shape s{};
    s.Mw = 4096; s.K = K; s.bits = bits; s.ts = 8; s.lay = 2;
    if (sm == 2) { s.gs = 0; s.ags = K; s.m_groups = 1; } else { s.gs = 64; s.ags = 64; s.m_groups = -1; }
    return s;
}

static void print_quad(bool ok, const QuadPlan& p) {
    if (!ok) { printf("refuse\n"); return; }
    printf("%d %d %d %d %d %d %d %d %d %d %d %zu | inst %d\n", p.ft, p.wpq, p.nr, (int)p.early, (int)p.dump, p.acc, p.lutsrc, (int)p.xf, (int)p.gn,
           (int)p.gt, p.gx, p.lds_bytes, (int)((p.xf || (!p.gn && !p.gt)) && quad_inst_exists(p.lutsrc, p.nr, p.ft, p.wpq, p.dump, p.acc, p.early, p.xf)));
}

int main() {
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        int bits, K, sm, tq, bl, du, ac, ft, wq, kind, strict, N;
        QuadPlan qp;
        if (sscanf(line, "q %d %d %d %d %d %d %d %d %d", &bits, &K, &sm, &tq, &bl, &du, &ac, &ft, &wq) == 9) {
            print_quad(quad_plan(shape(bits, K, sm), tq, bl != 0, du != 0, ac != 0, ft, wq, qp), qp);
        } else if (sscanf(line, "x %d %d %d %d %d %d %d %d", &bits, &K, &sm, &tq, &kind, &ft, &wq, &strict) == 8) {
            print_quad(quad_plan_xf(shape(bits, K, sm), tq, kind, ft, wq, strict != 0, qp), qp);
        } else if (sscanf(line, "r %d %d %d", &K, &N, &tq) == 3) {
            RowsLaunchPlan p;
            if (!rows_launch_plan(shape(2, K, 0), N, tq, p)) { printf("refuse\n"); continue; }
            printf("%d %d %d %d %zu %d", p.rows.r_fit, p.rows.ngroups, p.rows.cap_last, p.rows.live_last, p.rows.lds_bytes, p.wpq);
            bool inst = true;
            for (int i = 0; i < p.nlaunch; ++i) {
                printf(" | %d %d %d %d %zu", p.l[i].R, p.l[i].n_base, p.l[i].gx, p.l[i].gy, p.l[i].lds_bytes);
                inst = inst && rows_inst_exists(p.l[i].R);
            }
            printf(" | inst %d\n", (int)inst);
        } else if (sscanf(line, "p %d %d", &K, &N) == 2) {
            RowsPlan p;
            if (!rows_plan(K, N, p)) { printf("refuse\n"); continue; }
            printf("%d %d %d %d %zu\n", p.r_fit, p.ngroups, p.cap_last, p.live_last, p.lds_bytes);
        } else {
            printf("?\n");
        }
    }
    return 0;
}
