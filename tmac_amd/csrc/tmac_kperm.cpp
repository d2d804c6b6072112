// tmac_kperm.cpp — the K permutation of an act-order matrix from its g_idx: rules and layout in tmac_kperm.h.  Plain C++.
#include "tmac_kperm.h"

#include <cstring>

using namespace tmac_host;

uint64_t tmac_host::kperm_hash(const int32_t* perm, int K) {
    uint64_t h = 0xcbf29ce484222325ull;
    auto mix = [&](uint32_t v) {
        for (int b = 0; b < 4; ++b) { h ^= (v >> (8 * b)) & 0xffu; h *= 0x100000001b3ull; }
    };
    mix((uint32_t)K);
    for (int k = 0; k < K; ++k) mix((uint32_t)perm[k]);
    return h ? h : 1;
}

int32_t tmac_host::kperm_build(const int32_t* g_idx, int K, int group_size, KPermHost* out) {
    if (!g_idx || !out) return fail(TMAC_HIP_E_ARG, "null argument");
    if (K <= 0 || group_size <= 0) return fail(TMAC_HIP_E_ARG, "g_idx: K=%d and group_size=%d must be positive", K, group_size);
    if (K % group_size) return fail(TMAC_HIP_E_ARG, "g_idx: K=%d is no whole number of groups of %d", K, group_size);
    const int G = K / group_size;
    std::vector<int32_t> count((size_t)G, 0);
    for (int k = 0; k < K; ++k) {
        const int32_t g = g_idx[k];
        if (g < 0 || g >= G) return fail(TMAC_HIP_E_ARG, "g_idx[%d] = %d names group %d, outside [0, %d)", k, g, g, G);
        ++count[(size_t)g];
    }
    for (int g = 0; g < G; ++g)
        if (count[(size_t)g] != group_size)
            return fail(TMAC_HIP_E_ARG, "g_idx: group %d has %d members, not group_size = %d", g, count[(size_t)g], group_size);
    // every group has exactly group_size members: group g fills positions [g * group_size, (g + 1) * group_size) in the order its
    // members appear (stable)
    KPermHost p;
    p.K = K; p.gs = group_size;
    p.perm.assign((size_t)K, 0);
    std::vector<int32_t> next((size_t)G);
    for (int g = 0; g < G; ++g) next[(size_t)g] = g * group_size;
    p.identity = true;
    for (int k = 0; k < K; ++k) {
        const int32_t pos = next[(size_t)g_idx[k]]++;
        p.perm[(size_t)pos] = k;
        if (pos != k) p.identity = false;
    }
    p.id = kperm_hash(p.perm.data(), K);
    *out = std::move(p);
    return TMAC_HIP_OK;
}

bool tmac_host::kperm_equal(const KPermHost* a, const KPermHost* b) {
    if (a == b) return true;
    if (!a || !b) return false;
    return a->K == b->K && a->id == b->id && memcmp(a->perm.data(), b->perm.data(), sizeof(int32_t) * (size_t)a->K) == 0;
}
