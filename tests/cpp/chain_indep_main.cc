// The independence verdict of a recording (tmac_amd/csrc/tmac_chain_indep.h) as a stand-alone host program: no HIP, no device.
// tests/test_chain_indep_cpu.py builds it with g++.
//   chain_indep_main EXCHANGE_STEPS [src,src2,xf_kind,epi ...]      one quadruple per recorded call, in recorded order
//   stdout: why <tab> op <tab> other       (why: 0 independent, 1 flow, 2 flow of a GLU's second vector, 3 transform, 4 epilogue, 5 exchange)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../tmac_amd/csrc/tmac_chain_indep.h"

using namespace tmac_host;

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: see the head of chain_indep_main.cc\n"); return 2; }
    std::vector<IndepOp> ops;
    for (int i = 2; i < argc; ++i) {
        IndepOp o;
        if (sscanf(argv[i], "%d,%d,%d,%d", &o.src, &o.src2, &o.xf_kind, &o.epi) != 4) { fprintf(stderr, "bad call '%s'\n", argv[i]); return 2; }
        ops.push_back(o);
    }
    const IndepVerdict v = indep_verdict(ops.data(), ops.size(), (size_t)atoi(argv[1]));
    printf("%d\t%d\t%d\n", (int)v.why, v.op, v.other);
    return 0;
}
