// What a LUT workspace holds and the LUT build planner (tmac_amd/csrc/tmac_lut_held.h) as a stand-alone host program: no HIP, no device.
// tests/test_lut_held_cpu.py builds it with g++.
//   lut_held_main sweep maxK maxN
//       every request of the sweep below, one line each, tab-separated:
//       K N ags want mode unified pairs_min_n image_min_n image_buffers | rc | builder all_layouts row_image lut_image |
//       held: K N ags ref dev half image | then, of a LutHeld cleared and committed to the plan: serves_image(1 | 2, K, N),
//       serves_lut(K, ags, 1 | N | N + 1), built_through(id | 0 | id + 1), holds_exactly(K, N, ags), and whether any query
//       answers true after clear().  A refused request prints its message after rc and nothing else.
//       mode: 0 plain, 1 through a permutation (id 77, built for K), 2 with a transform (3: both, "plan" only).  image_min_n -1 = never.
//   lut_held_main plan K N ags want mode unified pairs_min_n image_min_n image_buffers maxK maxN perm_K
//       one request, the same line
#include <climits>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../tmac_amd/csrc/tmac_lut_held.h"

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
constexpr uint64_t PERM_ID = 77;

static bool any_query(const LutHeld& h, int K, int N, int ags) {
    bool any = h.holds_exactly(K, N, ags) || h.has_layout(LUT_REF) || h.has_layout(LUT_DEV) || h.has_layout(LUT_HALF);
    for (int n = 1; n <= N; ++n) any = any || h.serves_lut(K, ags, n) || h.serves_image(IMG_ROWWISE, K, n) || h.serves_image(IMG_CHUNK, K, n);
    for (uint64_t id : {(uint64_t)0, PERM_ID}) any = any || h.built_through(id);
    return any;
}

static void one(int K, int N, int ags, int want, int mode, int unified, int pmin, int thr, int bufs, int maxK, int maxN, int perm_K) {
    LutBuildReq q;
    q.K = K; q.N = N; q.ags = ags; q.want = (LutBuild)want; q.unified = unified != 0; q.xf = mode >= 2;
    if (mode == 1 || mode == 3) { q.perm_id = PERM_ID; q.perm_K = perm_K; }
    LutBuildCaps c;
    c.pairs_min_n = pmin; c.image_min_n = thr < 0 ? INT_MAX : thr; c.image_buffers = bufs != 0; c.maxK = maxK; c.maxN = maxN;
    LutBuildPlan p;
    const int32_t rc = lut_build_plan(q, c, &p);
    printf("%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t|\t%d\t", K, N, ags, want, mode, unified, pmin, thr, bufs, rc);
    if (rc) { printf("%s\n", g_msg.c_str()); return; }
    LutHeld h;
    h.commit(p);          // (a workspace's own sequence: clear, launches, commit)
    const LutHeld& ph = p.held;
    printf("|\t%d\t%d\t%d\t%d\t|\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t|\t", (int)p.builder, (int)p.all_layouts, (int)p.row_image, (int)p.lut_image, ph.K(), ph.N(), ph.ags(),
           (int)ph.has_layout(LUT_REF), (int)ph.has_layout(LUT_DEV), (int)ph.has_layout(LUT_HALF), (int)ph.image());
    printf("%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t", (int)h.serves_image(IMG_ROWWISE, K, N), (int)h.serves_image(IMG_CHUNK, K, N), (int)h.serves_lut(K, ags, 1),
           (int)h.serves_lut(K, ags, N), (int)h.serves_lut(K, ags, N + 1), (int)h.built_through(q.perm_id), (int)h.built_through(q.perm_id ? 0 : PERM_ID),
           (int)h.built_through(q.perm_id + 1), (int)h.holds_exactly(K, N, ags));
    h.clear();
    printf("%d\n", (int)any_query(h, K, N, ags));
}

int main(int argc, char** argv) {
    if (argc == 4 && !strcmp(argv[1], "sweep")) {
        const int maxK = atoi(argv[2]), maxN = atoi(argv[3]);
        for (int K : {64, 256, 1024, 12288, 12352})
            for (int N : {1, 2, 11, 12, 13, 70})
                for (int ags : {32, 64, K})
                    for (int want : {(int)LB_ALL, (int)LB_HALF_TABLES, (int)LB_IMAGE})
                        for (int mode : {0, 1, 2})
                            for (int unified : {0, 1})
                                for (int pmin : {2, 100})
                                    for (int thr : {12, 4, -1})
                                        for (int bufs : {1, 0}) one(K, N, ags, want, mode, unified, pmin, thr, bufs, maxK, maxN, K);
        return 0;
    }
    if (argc == 14 && !strcmp(argv[1], "plan")) {
        int a[12];
        for (int i = 0; i < 12; ++i) a[i] = atoi(argv[2 + i]);
        one(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10], a[11]);
        return 0;
    }
    fprintf(stderr, "usage: see the head of lut_held_main.cc\n");
    return 2;
}
