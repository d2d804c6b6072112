// The K permutation of act-order matrices (tmac_amd/csrc/tmac_kperm.cpp) as a stand-alone host program: no HIP, no device.
// tests/test_kperm_cpu.py builds it with g++.
//   kperm_main build K group_size g_idx.bin perm.bin     stdout: rc <tab> message <tab> identity <tab> id      (perm.bin written on success)
//   kperm_main equal K group_size a.bin b.bin            stdout: equal(0|1) <tab> id_a <tab> id_b              (both must build)
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../tmac_amd/csrc/tmac_kperm.h"

static std::string g_msg;
int32_t tmac_host::fail(int32_t code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_msg = buf;
    return code;
}

using namespace tmac_host;

static std::vector<int32_t> slurp(const char* path, int K) {
    std::vector<int32_t> v((size_t)(K > 0 ? K : 0));
    FILE* f = fopen(path, "rb");
    if (!f || (K > 0 && fread(v.data(), 4, (size_t)K, f) != (size_t)K)) { fprintf(stderr, "cannot read %d values from %s\n", K, path); exit(2); }
    fclose(f);
    return v;
}

int main(int argc, char** argv) {
    if (argc != 6) { fprintf(stderr, "usage: see the head of kperm_main.cc\n"); return 2; }
    const int K = atoi(argv[2]), gs = atoi(argv[3]);
    if (!strcmp(argv[1], "build")) {
        const std::vector<int32_t> g = slurp(argv[4], K);
        KPermHost p;
        const int32_t rc = kperm_build(g.data(), K, gs, &p);
        printf("%d\t%s\t%d\t%llu\n", rc, rc ? g_msg.c_str() : "", rc ? 0 : (int)p.identity, rc ? 0ull : (unsigned long long)p.id);
        if (rc == 0) {
            FILE* f = fopen(argv[5], "wb");
            if (!f || fwrite(p.perm.data(), 4, (size_t)K, f) != (size_t)K) { fprintf(stderr, "cannot write %s\n", argv[5]); return 2; }
            fclose(f);
        }
        return 0;
    }
    const std::vector<int32_t> ga = slurp(argv[4], K), gb = slurp(argv[5], K);
    KPermHost a, b;
    if (kperm_build(ga.data(), K, gs, &a) || kperm_build(gb.data(), K, gs, &b)) { fprintf(stderr, "build failed: %s\n", g_msg.c_str()); return 2; }
    printf("%d\t%llu\t%llu\n", (int)(kperm_equal(&a, &b) && kperm_equal(&b, &a) && kperm_equal(&a, &a)), (unsigned long long)a.id, (unsigned long long)b.id);
    return 0;
}
