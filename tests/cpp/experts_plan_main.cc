// experts_plan of tmac_amd/csrc/tmac_launch_plan.cpp as a stand-alone program (tests/test_experts_cpu.py): one query per line of stdin,
//   K bits gs Mw0 Mw1 S lut_rows mode          (Mw1 = 0: one bank; mode 0 SLOTS, 1 COMBINE)
// one answer per line of stdout: "wpq gx items lds_bytes | inst 0|1" (the policy predicate of the instantiation the plan names), or
// "refuse: <why>".
#include <stdio.h>

#include "../../tmac_amd/csrc/tmac_launch_plan.h"

using namespace tmac;

int main() {
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        int K, bits, gs, Mw[2], S, lut_rows, mode;
        if (sscanf(line, "%d %d %d %d %d %d %d %d", &K, &bits, &gs, &Mw[0], &Mw[1], &S, &lut_rows, &mode) != 8) { printf("?\n"); continue; }
        Shape s{};
        s.K = K; s.bits = bits; s.gs = gs; s.ags = 64; s.m_groups = -1; s.zero_point = 1; s.ts = 8; s.lay = 2;
        ExpertsPlan p;
        if (!experts_plan(s, Mw, Mw[1] ? 2 : 1, S, lut_rows, mode, p)) { printf("refuse: %s\n", p.why); continue; }
        printf("%d %d %d %zu | inst %d\n", p.wpq, p.gx, p.items, p.lds_bytes, (int)experts_inst_exists(bits, 0, mode));
    }
    return 0;
}
