// experts_rows_sizes of tmac_amd/csrc/tmac_launch_plan.cpp as a stand-alone program (tests/test_experts_rows_cpu.py): one query per line of
// stdin, "sizes N S E"; one answer per line of stdout: "T_max P" or "refuse: <why>".
#include <stdio.h>

#include "../../tmac_amd/csrc/tmac_launch_plan.h"

using namespace tmac;

int main() {
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        long long n, sl, e;
        if (sscanf(line, "sizes %lld %lld %lld", &n, &sl, &e) != 3) { printf("?\n"); continue; }
        ExpertsRowsSizes z;
        if (!experts_rows_sizes(n, sl, e, z)) printf("refuse: %s\n", z.why);
        else printf("%d %d\n", z.T_max, z.P);
    }
    return 0;
}
