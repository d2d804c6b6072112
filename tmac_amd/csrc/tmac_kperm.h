// tmac_kperm.h — the K permutation of an act-order (desc_act) GPTQ matrix: host logic.  No HIP header: tests/cpp/kperm_main.cc builds
// tmac_kperm.cpp with plain g++ (tests/test_kperm_cpu.py); the C-ABI around it (device copies, the object's lifetime) is at the foot of
// tmac_kperm.cpp, compiled only into the library.
//
// An act-order matrix is a group-quantised matrix whose K axis is permuted: perm = stable_argsort(g_idx) puts the columns of group 0
// first, then group 1, ... -- q[:, perm] lies in contiguous groups of group_size, scales and zeros are already in group order, and
// y = W x = W' x[perm].  perm[k'] is the SOURCE column (and activation) of position k' of the permuted matrix.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/tmac_hip.h"

namespace tmac_host {

int32_t fail(int32_t code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));   // tmac_runtime.cpp

struct KPermHost {
    int K = 0, gs = 0;
    bool identity = false;          // perm[k'] == k' throughout: what every non-act-order exporter writes (g_idx == k / group_size)
    uint64_t id = 0;                // 64-bit content hash of (K, perm); never 0 (0 is "no permutation" in the workspace's record)
    std::vector<int32_t> perm;      // [K], every value < K, each exactly once
};

// perm from g_idx (host copy, K values): a stable counting sort by group.  TMAC_HIP_OK, or fail(TMAC_HIP_E_ARG, ...) naming the first
// offending group: K % group_size != 0, a value outside [0, K / group_size), a group without exactly group_size members.
int32_t kperm_build(const int32_t* g_idx, int K, int group_size, KPermHost* out);
// FNV-1a over K and the K values
uint64_t kperm_hash(const int32_t* perm, int K);
// the same permutation: one object, or K, hash AND contents equal (memcmp: the hash alone does not decide)
bool kperm_equal(const KPermHost* a, const KPermHost* b);

}  // namespace tmac_host
