// tmac_chain_indep.h — are the calls of a recording independent of each other, and if not, which call says so first.  Plain C++ over
// host data (no HIP header): tmac_chain_host.cpp decides stream mode with it and words the refusal of a recording that was declared
// independent (tmac_hip_chain_begin_independent); tests/cpp/chain_indep_main.cc builds it with g++ (tests/test_chain_indep_cpu.py).
#pragma once
#include <cstddef>

namespace tmac_host {

// what the analysis of a recording knows about one call
struct IndepOp {
    int src;         // the earlier call whose output this call's activations are (-1: a vector in memory)
    int src2;        // ... the second vector of its GLU
    int xf_kind;     // its vector transform (0: none)
    int epi;         // it publishes gate(gate) * up for a later call (GLU in the producer)
};
enum IndepWhy { INDEP_OK = 0, INDEP_FLOW, INDEP_FLOW2, INDEP_XFORM, INDEP_EPILOGUE, INDEP_EXCHANGE };
struct IndepVerdict {
    IndepWhy why;    // INDEP_OK: stream mode may run these calls
    int op;          // the first call (in recorded order) that is not independent; -1 for INDEP_OK and INDEP_EXCHANGE
    int other;       // INDEP_FLOW / INDEP_FLOW2: the earlier call whose output it reads; else -1
};
// Calls are looked at in recorded order and a call's data flow before its transform; exchange steps, which belong to no call, last.
inline IndepVerdict indep_verdict(const IndepOp* ops, size_t n, size_t exchange_steps) {
    for (size_t i = 0; i < n; ++i) {
        if (ops[i].src >= 0) return IndepVerdict{INDEP_FLOW, (int)i, ops[i].src};
        if (ops[i].src2 >= 0) return IndepVerdict{INDEP_FLOW2, (int)i, ops[i].src2};
        if (ops[i].xf_kind != 0) return IndepVerdict{INDEP_XFORM, (int)i, -1};
        if (ops[i].epi) return IndepVerdict{INDEP_EPILOGUE, (int)i, -1};
    }
    if (exchange_steps) return IndepVerdict{INDEP_EXCHANGE, -1, -1};
    return IndepVerdict{INDEP_OK, -1, -1};
}

}  // namespace tmac_host
