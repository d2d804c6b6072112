// tmac_launch_plan.h — launch planning: which configuration and which instantiation of a kernel a call runs, decided on the host in plain
// C++ (no HIP header: g++ compiles tmac_launch_plan.cpp on its own, tests/test_launch_plan_cpu.py).  Per kernel family:
//   * a `constexpr` POLICY PREDICATE: which template-argument combinations exist.  The selectors (tmac_select.h) instantiate what passes it
//     and nothing else; the planners refuse what fails it.
//   * a PLAN struct and a pure function that fills it or refuses -- it reads its arguments and nothing else.
// The launcher in the .hip file is: plan, select the template arguments from the plan's fields, launch.  DESIGN.md 4.2, 4.8.
#pragma once
#include <stddef.h>

#include "tmac_layout.h"

namespace tmac {

// ---- shapes the fused kernels take ------------------------------------------------------------------------------------------------
bool gemv_fused_supported(const Shape& s);      // k_gemv_fused (tmac_fused.hip)
bool gemv_quad_supported(const Shape& s);       // k_gemv_quad (tmac_quad.hip)

// the host-side divides of a FusedArgs / FusedXfArgs (filled by the launchers)
template <class Args>
inline void fused_precompute(Args& a) {
    const Shape& s = a.s;
    a.nu = s.K / 32;
    a.nsb = (a.nu + KL - 1) / KL;
    a.tstride = ((a.nu + 15) & ~15) + 1;
    a.G = s.K / s.ags;
    a.nsg = s.gs > 0 ? s.K / s.gs : 1;
    a.gs_shift = 0;
    if (s.gs > 0) for (int g = s.gs / 32; g > 1; g >>= 1) ++a.gs_shift;
}

// ---- k_gemv_quad --------------------------------------------------------------------------------------------------------------------
// The (threads, waves per quad) configurations of the kernel, and the four the XF instantiations cover -- one per waves-per-quad count,
// which is what shapes the K walk and the cross-wave reductions -- so that eight translation units grow by 12 kernels per scale flavour
// instead of 20.
constexpr bool quad_config_exists(int ft, int wpq) {
    return (ft == 512 && (wpq == 1 || wpq == 2)) || (ft == 768 && wpq >= 1 && wpq <= 3) || (ft == 1024 && (wpq == 1 || wpq == 2 || wpq == 4));
}
constexpr bool quad_xf_covered(int ft, int wpq) { return (ft == 512 && (wpq == 1 || wpq == 2)) || (ft == 768 && wpq == 3) || (ft == 1024 && wpq == 4); }
// Instantiation policy of k_gemv_quad<BITS, ZP, SM, LUTSRC, NR, FT, WPQ, DUMP, ACC, SCF16, EARLY, XF, GN, GT> (BITS, ZP, SM, SCF16: by translation
// unit and scale flavour; GN, GT: every XF form has all four; GA and BI: quad_ga_inst_exists, quad_bi_inst_exists below):
//   * NR is 2 or 6 tables per thread; 6 only where the kernel builds the LUT (LUTSRC 1) -- a copied image has no build to spread;
//   * the v_mqsad accumulate (ACC 0, A/B variant 7), the prebuilt-LUT source (LUTSRC 0) and the integer tap (DUMP) exist for 512-thread
//     workgroups only, and without EARLY;
//   * 768- and 1024-thread workgroups exist with EARLY alone (grids of these sizes never exceed one workgroup per CU);
//   * the transform (XF) lives in the in-kernel LUT build of the MFMA form, in the covered configurations.
constexpr bool quad_inst_exists(int lutsrc, int nr, int ft, int wpq, bool dump, int acc, bool early, bool xf) {
    if (!quad_config_exists(ft, wpq) || (nr != 2 && nr != 6) || (nr == 6 && lutsrc != 1)) return false;
    const bool production = lutsrc == 1 && acc == 1 && !dump;
    if (xf) return production && quad_xf_covered(ft, wpq) && (early || ft == 512);
    return ft == 512 ? (!early || production) : (production && early);
}

// The gather of an act-order permutation (GA) lives where the transform lives -- the in-kernel LUT build of the MFMA form, in the covered
// configurations, no tap -- and never together with one.
constexpr bool quad_ga_inst_exists(int nr, int ft, int wpq, bool early) { return quad_inst_exists(1, nr, ft, wpq, false, 1, early, true); }

// The bias add (BI) lives at the store of the MFMA form, per-group scales, no tap.  LUT built in-kernel: where the transform and the gather
// live (with a transform: NORM and the silu GLU, i.e. neither GN nor GT).  LUT copied from the workspace's image (the row loop behind a
// half-table build, the split entry point): what the plain kernel has there -- 512-thread workgroups, two tables per thread, no EARLY.
constexpr bool quad_bi_inst_exists(int lutsrc, int nr, int ft, int wpq, bool early, bool xf) {
    if (lutsrc == 0) return !xf && quad_xf_covered(ft, wpq) && quad_inst_exists(0, nr, ft, wpq, false, 1, early, false);
    return quad_inst_exists(1, nr, ft, wpq, false, 1, early, true);
}

struct QuadPlan {
    int ft, wpq;             // threads, waves per quad
    int nr;                  // tables built per thread (2 | 6)
    bool early;              // weight fragments issued before the LUT build: at most one workgroup per CU
    bool dump;               // the integer tap
    int acc, lutsrc;         // 1 MFMA / 0 v_mqsad accumulate; 1 LUT built in-kernel / 0 copied image
    bool xf, gn, gt;         // vector transform; its GLU_NORM form; its gate a run-time choice
    int gx;                  // grid (x)
    size_t lds_bytes;
    bool ga;                 // the gather of an act-order permutation in the activation loads (never with xf)
    bool bi;                 // the bias add at the store (never with ga, gn, gt, dump or the v_mqsad accumulate)
};
constexpr int QUAD_XF_MAX_K = 24576;
size_t quad_lds_bytes(const Shape& s, int nwv);
// The (threads, waves per quad) of a launch: best_ft / best_wpq; false when the kernel has no such configuration.  need512: the launch
// wants an instantiation that exists for 512-thread workgroups only (tap, prebuilt LUT, v_mqsad accumulate).  force_*: 0 = heuristic.
bool quad_config(const Shape& s, bool need512, int total_q, int force_ft, int force_wpq, int& best_ft, int& best_wpq);
// total_q: row quads of all matrices.  false: refused (launch_gemv_quad's overloads then return hipErrorInvalidValue).
bool quad_plan(const Shape& s, int total_q, bool build_lut, bool dump, bool acc_mfma, int force_ft, int force_wpq, QuadPlan& p);
// xf_kind: tmac_hip_xform::kind as it comes (kind | gate << 8).  strict: the configuration was forced by the caller and must be covered as
// it is; else one outside the covered set falls back to the nearest covered one.
bool quad_plan_xf(const Shape& s, int total_q, int xf_kind, int force_ft, int force_wpq, bool strict, QuadPlan& p);
// the gather instantiations: quad_plan_xf's configuration rule (covered set, fall-back, strict), per-group scales only
bool quad_plan_perm(const Shape& s, int total_q, int force_ft, int force_wpq, bool strict, QuadPlan& p);
// The bias instantiations, per-group scales only.  build_lut: quad_plan_xf's configuration rule (covered set, fall-back, strict); xf_kind 0 =
// no transform, else NORM or the silu GLU (anything else is refused).  !build_lut (never with a transform): the 512-thread configuration the
// plain copy form takes -- a forced one outside (512,1) / (512,2) is refused as it is for the plain block.
bool quad_plan_bias(const Shape& s, int total_q, bool build_lut, int xf_kind, int force_ft, int force_wpq, bool strict, QuadPlan& p);

// ---- k_gemv_rows --------------------------------------------------------------------------------------------------------------------
constexpr int ROWS_FT = 512, ROWS_NWV = ROWS_FT / 64;
constexpr bool rows_inst_exists(int r) { return r == 2 || r == 4 || r == 8; }      // k_gemv_rows<..., R>: the row capacity of a workgroup
// The row groups of N rows (pure): r_fit = largest of 8 / 4 / 2 whose LDS footprint fits 160 KiB (0: none); every group but the last
// holds r_fit rows (capacity r_fit), the last the remainder in the smallest capacity of 2 / 4 / 8 that takes it.
struct RowsPlan { int r_fit, ngroups, cap_last, live_last; size_t lds_bytes; };   // lds_bytes: of a capacity-r_fit workgroup
constexpr size_t ROWS_LDS_MAX = 163840;
size_t rows_lds_bytes(int K, int R);
bool rows_plan(int K, int N, RowsPlan& p);       // false: K % 64, N < 1, or not even two rows fit
bool gemv_rows_supported(const Shape& s);
// The launches of a call: one for the groups of capacity r_fit (blockIdx.y = group), one for a last group of another capacity.
struct RowsLaunch { int R, n_base, gx, gy; size_t lds_bytes; };
struct RowsLaunchPlan { RowsPlan rows; int wpq; int nlaunch; RowsLaunch l[2]; };
bool rows_launch_plan(const Shape& s, int N, int total_q, RowsLaunchPlan& p);

// ---- k_decode_chain<BITS, ZP, SCF16, SM, XF, TAP, G2, GT> ---------------------------------------------------------------------------
// The tap's instance carries the transforms too, and a gate other than silu belongs to a transform: TAP and GT imply XF.  Unified scales
// (SM 2) have one scale per matrix: no G2 instance (two scale groups per lane and item), and no zero points.
constexpr bool chain_inst_exists(bool zp, int sm, bool xf, bool tap, bool g2, bool gt) {
    return (sm == 0 || (sm == 2 && !zp && !g2)) && (xf || (!tap && !gt));
}

// ---- k_gemv_stream<BITS, ZP, SCF16, RING, MW, SM, TAP, QW, G2> ----------------------------------------------------------------------
// Ring depths.  Two workgroups share a CU only with <= 64 VGPRs per wave; a G2 fragment is one or two registers larger, and where the
// ring of the nsplit >= 2 instance would pass 64 with it the ring gets shallower (never a spill: a spill behind the ring waits for the
// weights) -- 3-bit G2: one fragment, as 4-bit weights have at nsplit >= 2.  4-bit G2 has no ring left to give: a launch with nsplit >= 2
// runs the one-workgroup instance there (the workgroups then do not share a CU; nothing in the kernel depends on that).  The host's
// nsplit rule for G2 follows (plan_stream).
struct StreamInst { int ring, mw; };      // weight fragments in flight per wave; the MW argument: 8 = two workgroups per CU, 4 = one
constexpr StreamInst stream_inst(int bits, bool g2, int nsplit, bool tap) {
    if (nsplit >= 2 && !tap && !(g2 && bits == 4)) return {g2 ? (bits <= 2 ? 2 : 1) : (bits <= 3 ? 2 : 1), 8};      // <= 64 VGPRs
    return {bits <= 2 ? 4 : 2, 4};      // one workgroup per CU: ring depth 2..8 measured flat (profiles/r05_stream_knockouts.txt); the tap's instance
}
// Ring and waves are stream_inst's and nothing else's (the launcher instantiates no other pair); what is left to exclude is the scale
// flavour: unified scales have no zero points (qgemm.py:170-174) and no G2 instance
constexpr bool stream_inst_exists(bool zp, int sm, bool g2) { return sm == 0 || (sm == 2 && !zp && !g2); }

}  // namespace tmac
