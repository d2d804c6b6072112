// tmac_lut_held.h — what a LUT workspace holds, and which launches put it there: host logic.  No HIP header: tests/cpp/lut_held_main.cc
// builds it with plain g++ (tests/test_lut_held_cpu.py).
//
// A workspace has three LUT layouts (qlut_ref, qlut_dev, the half-table image qlut_lds; lut_scales / lut_biases go with each) and the LUT
// image k_gemm_planes streams (gimg / gcol).  LutHeld says which of them the buffers hold, for which K x N activation rows, act group size
// and K permutation.  It changes in two ways only: clear() -- holds nothing -- and commit(plan), and tmac_workspace.cpp calls them in that
// order around the launches of a plan (lut_build, tmac_hip_workspace_write): a build that failed half way leaves a workspace that holds
// nothing.  Readers ask the queries; nobody compares fields.
//
// lut_build_plan is the one place that chooses the builder: a pure function of the request (what the entry point wants) and the caps (the
// knobs and the workspace, read once by the caller).
#pragma once
#include <climits>
#include <cstddef>
#include <cstdint>

#include "../../include/tmac_hip.h"
#include "tmac_layout.h"

namespace tmac_host {

int32_t fail(int32_t code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));   // tmac_runtime.cpp

constexpr int PAIRS_ROW_MAX_K = 12288;   // largest K of the row-wise pair build (k_preprocess_pairs_row) and so of the row-wise LUT image
inline size_t qdev_u4_for_K(int K) { return (size_t)((K / (4 * tmac::TS) + tmac::KL - 1) / tmac::KL) * 8 * tmac::KL; }   // uint4 per activation row of qlut_dev

enum LutLayout : unsigned { LUT_REF = 1, LUT_DEV = 2, LUT_HALF = 4, LUT_ALL_LAYOUTS = 7 };
// the LUT image: row-wise (one act group per row, k_gemm_planes_us) | chunk-major (act groups of 64, k_gemm_planes)
enum LutImage { IMG_NONE = 0, IMG_ROWWISE = 1, IMG_CHUNK = 2 };
// what an entry point wants built (the fused entry point's plans name one; the preprocessor entry points want LB_ALL)
enum LutBuild {
    LB_NONE,         // none: the GEMV kernel builds its own
    LB_IMAGE,        // k_gemm_planes' LUT image alone
    LB_HALF_TABLES,  // the half-table image (qlut_lds) alone, two tables per lane: all that k_gemm_onehot, k_gemv_quad and k_gemv_rows read
    LB_ALL           // every layout of the workspace, and the LUT image where tmac_hip_qgemm_dev may pick k_gemm_planes
};
enum LutBuilder { LUTB_NONE, LUTB_PREPROCESS, LUTB_PAIRS, LUTB_PAIRS_ROW };   // k_preprocess | k_preprocess_pairs | k_preprocess_pairs_row

struct LutBuildReq {
    int K = 0, N = 0, ags = 0;
    LutBuild want = LB_ALL;
    bool unified = false;      // unified weight scales (one act group per row): decides the image kind of LB_IMAGE only
    bool xf = false;           // the build carries a vector transform
    uint64_t perm_id = 0;      // the build gathers through this K permutation (0 = none) ...
    int perm_K = 0;            // ... which was built for this K
};
struct LutBuildCaps {
    int pairs_min_n = 2;       // rows from which LB_ALL uses the pair builds (Knobs::pairs_min_n)
    int image_min_n = 12;      // rows from which LB_ALL also builds the LUT image; INT_MAX = never (k_gemm_onehot selected, GEMMs off)
    bool image_buffers = false;
    int maxK = 0, maxN = 0;
};
struct LutBuildPlan;

class LutHeld {
public:
    int K() const { return K_; }
    int N() const { return N_; }
    int ags() const { return ags_; }
    LutImage image() const { return image_; }
    size_t qdev_u4_per_row() const { return qdev_u4_for_K(K_); }
    bool has_layout(LutLayout l) const { return (layouts_ & l) != 0; }
    // rows 0 .. N - 1 of a LUT (any layout) of this K and act group size
    bool serves_lut(int K, int ags, int N) const { return layouts_ && K == K_ && ags == ags_ && N >= 1 && N <= N_; }
    // ... of the LUT image of this kind; it is by construction the image of the rows the layouts were built from
    bool serves_image(LutImage kind, int K, int N) const { return kind != IMG_NONE && kind == image_ && K == K_ && N >= 1 && N <= N_; }
    // something is held, and it was built through this K permutation (0: through none)
    bool built_through(uint64_t perm_id) const { return (layouts_ || image_ != IMG_NONE) && perm_id == perm_id_; }
    // the reference layout of exactly these rows (tmac_hip_workspace_read)
    bool holds_exactly(int K, int N, int ags) const { return has_layout(LUT_REF) && K == K_ && N == N_ && ags == ags_; }

    void clear() { *this = LutHeld(); }
    inline void commit(const LutBuildPlan& p);

private:
    friend int32_t lut_build_plan(const LutBuildReq&, const LutBuildCaps&, LutBuildPlan*);
    friend LutBuildPlan lut_write_plan(int K, int N, int ags);
    int K_ = 0, N_ = 0, ags_ = 0;
    unsigned layouts_ = 0;
    LutImage image_ = IMG_NONE;
    uint64_t perm_id_ = 0;
};

struct LutBuildPlan {
    LutBuilder builder = LUTB_NONE;
    bool all_layouts = false;   // the builder writes qlut_ref and qlut_dev next to the half-table image
    bool row_image = false;     // LUTB_PAIRS_ROW also writes the row-wise LUT image
    bool lut_image = false;     // k_lut_image runs after the builder: the chunk-major LUT image
    LutHeld held;               // what the workspace holds once every launch of the plan is enqueued
};
inline void LutHeld::commit(const LutBuildPlan& p) { *this = p.held; }

// K, N and the act group size of any LUT in a workspace of maxK x maxN
inline int32_t lut_shape_check(int K, int N, int ags, int maxK, int maxN) {
    if (K <= 0 || K > maxK || N <= 0 || N > maxN) return fail(TMAC_HIP_E_ARG, "K=%d N=%d exceed the workspace (%d, %d)", K, N, maxK, maxN);
    if (ags <= 0 || ags % 32 || K % ags) return fail(TMAC_HIP_E_NOMATCH, "act_group_size=%d must be a multiple of 32 dividing K=%d (qgemm.py:402-404)", ags, K);
    if (K % 64) return fail(TMAC_HIP_E_NOMATCH, "K=%d must be a multiple of 64", K);
    return TMAC_HIP_OK;
}

// The launches that serve a request, and what the workspace holds after them.  TMAC_HIP_OK and *out, or fail(code, ...).  Pure.
inline int32_t lut_build_plan(const LutBuildReq& q, const LutBuildCaps& c, LutBuildPlan* out) {
    const int32_t rc = lut_shape_check(q.K, q.N, q.ags, c.maxK, c.maxN);
    if (rc) return rc;
    const bool perm = q.perm_id != 0;
    // the gather lives in k_preprocess_pairs and k_lut_image, the transform in the builds of one layout
    if (perm && q.ags != 64) return fail(TMAC_HIP_E_NOMATCH, "the gathered LUT build takes act groups of 64 (act_group_size=%d)", q.ags);
    if (perm && q.perm_K != q.K) return fail(TMAC_HIP_E_ARG, "the K permutation was built for K=%d; the call has K=%d", q.perm_K, q.K);
    if (q.xf && q.want == LB_ALL)
        return fail(TMAC_HIP_E_NOMATCH, "a transformed call of several rows needs the LUT image or the half-table image alone; this plan builds every layout");
    if (q.xf && perm) return fail(TMAC_HIP_E_NOMATCH, "a LUT build takes a vector transform or a K permutation, not both");
    LutBuildPlan p;
    LutHeld& h = p.held;
    h.K_ = q.K; h.N_ = q.N; h.ags_ = q.ags; h.perm_id_ = q.perm_id;
    switch (q.want) {
    case LB_ALL: {
        // Several rows with act groups of 64: the pair-wise build, two tables per lane (a permutation: always, it has the gather).  One act
        // group per row: the row-wise pair build.  Otherwise one workgroup per act group: any group size, and cheap for a single row.
        const bool pairs = q.ags == 64 && (perm || q.N >= c.pairs_min_n);
        const bool pairs_row = !pairs && q.ags == q.K && q.K <= PAIRS_ROW_MAX_K && q.N >= c.pairs_min_n;
        p.builder = pairs ? LUTB_PAIRS : pairs_row ? LUTB_PAIRS_ROW : LUTB_PREPROCESS;
        p.all_layouts = true;
        h.layouts_ = LUT_ALL_LAYOUTS;
        // k_gemm_planes' LUT image, when tmac_hip_qgemm_dev may pick that kernel: not for one row, and not below the GEMM threshold
        // (PLANES_MIN_N by default: the matrix, and with it the measured crossover plan_split applies, is not known here).  Chunk-major for
        // act groups of 64, whatever built the layouts; row-wise from the row-wise pair build itself.  K == 64 is both: chunk-major wins,
        // the unified-scale GEMM is not offered it.
        const bool want_img = q.N >= 2 && q.N >= c.image_min_n && c.image_buffers;
        p.lut_image = want_img && q.ags == 64;
        p.row_image = want_img && pairs_row;
        h.image_ = p.lut_image ? IMG_CHUNK : p.row_image ? IMG_ROWWISE : IMG_NONE;
        break;
    }
    case LB_HALF_TABLES:
        p.builder = q.ags == 64 ? LUTB_PAIRS : LUTB_PAIRS_ROW;
        h.layouts_ = LUT_HALF;
        break;
    case LB_IMAGE:
        // The image alone: the workspace serves no LUT query afterwards (no layout is recorded, though the row-wise build passes through
        // qlut_lds).  The image IS recorded, with its rows: the plan says what the launches write, and no entry point can ask -- the fused
        // entry point, the only one that wants LB_IMAGE, launches k_gemm_planes on it itself and rebuilds on every call.
        p.builder = q.unified ? LUTB_PAIRS_ROW : LUTB_NONE;
        p.row_image = q.unified;
        p.lut_image = !q.unified;
        h.image_ = q.unified ? IMG_ROWWISE : IMG_CHUNK;
        break;
    default: return fail(TMAC_HIP_E_ARG, "no LUT build was asked for");
    }
    *out = p;
    return TMAC_HIP_OK;
}

// tmac_hip_workspace_write: the caller's LUT in every layout (no launch of a builder), no image, no permutation
inline LutBuildPlan lut_write_plan(int K, int N, int ags) {
    LutBuildPlan p;
    p.all_layouts = true;
    p.held.K_ = K; p.held.N_ = N; p.held.ags_ = ags; p.held.layouts_ = LUT_ALL_LAYOUTS;
    return p;
}

}  // namespace tmac_host
