// The transform resolver (tmac_amd/csrc/tmac_xform.cpp) as a stand-alone host program: no HIP, no device, pointers are plain integers
// and nothing is dereferenced.  tests/test_xf_resolve_cpu.py builds it with g++ and replays tests/golden/xf_refusals.json through it.
//
// stdin, one case per line:  site kind in2 residual gamma residual_out keep B_dev K N out out_bytes
//   site: xf | rows | tap | chain;  pointers as integers (0 = NULL, 1 = TMAC_XF_CARRY);  fp32 activations;  out: C_dev[0], the tap's x_out
// stdout, one line per case:  rc <tab> message
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../tmac_amd/csrc/tmac_xform.h"

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

static int32_t run(const char* site_name, const tmac_hip_xform& xf, const void* B, int K, int N, const void* out, size_t out_bytes) {
    const bool tap = !strcmp(site_name, "tap");
    const XfSite site = !strcmp(site_name, "chain") ? XF_SITE_CHAIN : !strcmp(site_name, "xf") ? XF_SITE_N1 : XF_SITE_ROWS;
    XfSpec s;
    const int32_t rc = xf_resolve(&xf, site, &s);
    if (rc || site == XF_SITE_CHAIN) return rc;
    const XfOut o{out, out_bytes};
    return xf_overlap_check(s, site, B, 4, xf.in2, K, N, &o, 1, tap ? "x_out_dev" : nullptr);
}

int main() {
    char site[16];
    long long kind, keep, K, N;
    unsigned long long in2, residual, gamma, rout, B, out, out_bytes;
    while (scanf("%15s %lld %llu %llu %llu %llu %lld %llu %lld %lld %llu %llu", site, &kind, &in2, &residual, &gamma, &rout, &keep, &B, &K, &N, &out, &out_bytes) == 12) {
        tmac_hip_xform xf;
        memset(&xf, 0, sizeof(xf));
        xf.kind = (int32_t)kind; xf.keep = (int32_t)keep; xf.eps = 1e-5f;
        xf.in2 = (const void*)(uintptr_t)in2; xf.residual = (const float*)(uintptr_t)residual;
        xf.gamma = (const float*)(uintptr_t)gamma; xf.residual_out = (float*)(uintptr_t)rout;
        g_msg.clear();
        const int32_t rc = run(site, xf, (const void*)(uintptr_t)B, (int)K, (int)N, (const void*)(uintptr_t)out, (size_t)out_bytes);
        printf("%d\t%s\n", rc, rc ? g_msg.c_str() : "");
    }
    return 0;
}
