// tmac_launch_plan.cpp — the launch planners of tmac_launch_plan.h.  Plain C++: no HIP header, no device code, no state.
#include "tmac_launch_plan.h"

namespace tmac {

bool gemv_fused_supported(const Shape& s) {
    if (s.bits < 1 || s.bits > 4 || s.K % 64 != 0 || s.K > 16384) return false;
    if (s.m_groups >= 1) return s.ags == s.K && s.Mw % s.m_groups == 0;
    const int gu = s.gs / 32;   // scale group in units; must be a power of two (shift instead of divide)
    return s.ags == 64 && s.gs >= 64 && s.gs % 64 == 0 && s.K % s.gs == 0 && (gu & (gu - 1)) == 0;
}

bool gemv_quad_supported(const Shape& s) {
    if (s.bits < 1 || s.bits > 4 || s.K % 64 != 0 || s.K > 24576 || s.Mw % 4 != 0) return false;
    if (s.m_groups >= 1) return s.ags == s.K && s.Mw % s.m_groups == 0;
    const int gu = s.gs / 32;
    return s.ags == 64 && s.gs >= 64 && s.gs % 64 == 0 && s.K % s.gs == 0 && (gu & (gu - 1)) == 0;
}

size_t quad_lds_bytes(const Shape& s, int nwv) {
    const int nu = s.K / 32, nst = (nu + 63) / 64, G = s.K / s.ags;
    return (size_t)4 * (nst * 64 + 1) * 16 + sizeof(float) * (2 * (nst * 32 > G ? nst * 32 : G) + 2 * nwv * 16 + nwv + s.K / 32);
}

bool quad_config(const Shape& s, bool need512, int total_q, int force_ft, int force_wpq, int& best_ft, int& best_wpq) {
    // Configuration choice, from tools/tune_quad.py on MI355X (profiles/r01_tune_quad.txt, us per launch in a graph):
    //   W2: o 4096x4096: (512,2) 4.3 | qkv 12288x4096: (512,2) 6.5, (512,1) 6.6, (1024,1) 6.9 | gate_up 22016x4096:
    //   (512,1) 9.2, (512,2) 10.2 | down 4096x11008: (768,3) 6.9, (1024,4) 7.2, (512,2) 7.3, (512,1) 8.8.
    //   W4 (tune_quad.py 0 4): o (512,2) | qkv (512,2) | gate_up (512,1) | down (512,2).
    const int BITS = s.bits;
    const int nst = (s.K / 32 + 63) / 64;
    // two waves per quad up to one quad per wave slot of the chip (4096), one beyond
    best_ft = 512; best_wpq = (total_q <= 4096 && nst >= 2) ? 2 : 1;
    // ... except where two waves per quad would leave the chip between one and two workgroups per CU (shards of a
    // row-split model: 3 x 2048 and 2 x 2752 rows measured 7 % faster with one, profiles/history/r01_autotune_shards_before_heuristic.txt)
    if (best_wpq == 2 && total_q > 1024 && total_q < 2048) best_wpq = 1;
    if (BITS == 2 && total_q <= 1024 && nst >= 4 && !need512) {
        // long rows, few quads: 3 waves per quad when that splits the steps evenly, else 4
        if (nst % 3 == 0 && s.K / 4 <= 6 * 768) { best_ft = 768; best_wpq = 3; }
        else { best_ft = 1024; best_wpq = 4; }
    }
    // One balanced pass: if twelve-wave workgroups with 1, 2 or 3 waves per quad cover the quads in a single pass over
    // 75-100 % of the CUs, every CU gets the same work, the LUT is built once per CU and the weights can be issued early.
    // Matches every case the tuner found on the llama-2-7B shapes and their 2-/4-/8-way row shards
    // (profiles/history/r01_autotune_shards_before_heuristic.txt and the runs after it): q/k/v 3 x 4096 rows -> (768,1) 5.6 against 6.1 us; 3 x 2048 -> (768,2);
    // gate/up 2 x 5504 -> (768,1) 5.45 against 5.9; 2 x 2752 -> (768,2); down 4096 x 11008 -> (768,3).
    if (!need512 && s.K / 4 <= 6 * 768) {
        for (int wq = 1; wq <= 3; ++wq) {
            if (wq > nst || nst % wq || (wq == 3 && BITS > 2)) continue;   // (W4 long rows measure better on (512,2): tune_quad.py 0 4)
            const int wgs = (total_q * wq + 11) / 12;
            if (wgs > 192 && wgs <= 256) { best_ft = 768; best_wpq = wq; break; }
        }
    }
    if (s.K / 4 > 6 * 512 && best_ft == 512 && !need512) best_ft = 1024;   // LUT build: <= 6 tables per thread
    if (force_ft) { best_ft = force_ft; if (!force_wpq && best_wpq > 2) best_wpq = 2; }
    if (force_wpq) best_wpq = force_wpq;
    if (best_ft == 768 || best_wpq == 3)          // 12 waves: 3 per quad (balanced when the row has 3k steps), or 12 / 6 quads per workgroup
        return best_ft == 768 && !need512 && s.K / 4 <= 6 * 768 && best_wpq >= 1 && best_wpq <= 3;
    // (six tables per thread is the limit of a launch that BUILDS the LUT: quad_plan_finish applies it there.  A launch that copies the
    // workspace's image has no build to spread and takes any K -- K = 14336, llama-3-8B's down projection, through the split entry point)
    return !((need512 && best_ft != 512) || (best_wpq == 4 && best_ft != 1024) || (best_ft != 512 && best_ft != 1024) ||
             (best_wpq != 1 && best_wpq != 2 && best_wpq != 4));
}

// grid, tables per thread, EARLY and LDS of a plan whose configuration and instantiation flags are set; false: no such instantiation
static bool quad_plan_finish(const Shape& s, int total_q, QuadPlan& p) {
    const int ipi = p.ft / 64 / p.wpq;
    p.lds_bytes = quad_lds_bytes(s, p.ft / 64);
    p.gx = (total_q + ipi - 1) / ipi;
    const int cap = (p.ft > 512) ? 256 : 512;       // persistent: <= 1 (FT = 768, 1024) / 2 (FT = 512) workgroups per CU (measured best)
    if (p.gx > cap) p.gx = cap;
    const int T = s.K / 4;
    const bool two = (p.lutsrc == 0 || T <= 2 * p.ft);
    if (!two && T > 6 * p.ft) return false;
    p.nr = two ? 2 : 6;
    // one workgroup per CU: overlap the weight stream with the LUT build (see the kernel); grids of the 768- and 1024-thread
    // configurations never exceed one workgroup per CU
    p.early = p.ft != 512 || (p.lutsrc == 1 && p.acc == 1 && !p.dump && p.gx <= 256);
    if (p.ga) return quad_ga_inst_exists(p.nr, p.ft, p.wpq, p.early);
    if (p.bi) return quad_bi_inst_exists(p.lutsrc, p.nr, p.ft, p.wpq, p.early, p.xf);
    return quad_inst_exists(p.lutsrc, p.nr, p.ft, p.wpq, p.dump, p.acc, p.early, p.xf);
}

bool quad_plan(const Shape& s, int total_q, bool build_lut, bool dump, bool acc_mfma, int force_ft, int force_wpq, QuadPlan& p) {
    p = QuadPlan{};
    if (!gemv_quad_supported(s)) return false;
    p.lutsrc = build_lut ? 1 : 0; p.dump = dump; p.acc = acc_mfma ? 1 : 0;
    if (!quad_config(s, dump || !build_lut || !acc_mfma, total_q, force_ft, force_wpq, p.ft, p.wpq)) return false;
    return quad_plan_finish(s, total_q, p);
}

// the configuration of an XF or GA launch: the heuristic's (or the forced one) where the instantiations cover it, else the fall-back below
static bool quad_config_covered(const Shape& s, int total_q, int force_ft, int force_wpq, bool strict, QuadPlan& p) {
    if (!quad_config(s, false, total_q, force_ft, force_wpq, p.ft, p.wpq)) return false;
    // A configuration the caller forced (tmac_hip_debug_quad_config) outside the covered set is refused; one the heuristic or the tuned table
    // chose falls back to the nearest covered one: same waves per quad in 512-thread workgroups ((768,1), (1024,1) -> (512,1); (768,2),
    // (1024,2) -> (512,2)), or (1024,4) where 512 threads cannot build the tables (K > 12288: more than six per thread).
    if (!quad_xf_covered(p.ft, p.wpq)) {
        if (strict) return false;
        if (s.K / 4 > 6 * 512) { p.ft = 1024; p.wpq = 4; }
        else { p.ft = 512; p.wpq = p.wpq >= 2 ? 2 : 1; }
    }
    return true;
}

bool quad_plan_xf(const Shape& s, int total_q, int xf_kind, int force_ft, int force_wpq, bool strict, QuadPlan& p) {
    p = QuadPlan{};
    if (!gemv_quad_supported(s) || s.K > QUAD_XF_MAX_K) return false;
    p.lutsrc = 1; p.acc = 1; p.xf = true;
    if (!quad_config_covered(s, total_q, force_ft, force_wpq, strict, p)) return false;
    // GLU_NORM has instantiations of its own (GN): the ones NORM and GLU run on stay as they were; and relu^2 and GELU have theirs (GT), next
    // to both: a call with silu runs what it ran
    p.gn = (xf_kind & 0xff) == 4; p.gt = (xf_kind >> 8) != 0;
    return quad_plan_finish(s, total_q, p);
}

bool quad_plan_perm(const Shape& s, int total_q, int force_ft, int force_wpq, bool strict, QuadPlan& p) {
    p = QuadPlan{};
    if (!gemv_quad_supported(s) || s.m_groups >= 1 || s.K > QUAD_XF_MAX_K) return false;
    p.lutsrc = 1; p.acc = 1; p.ga = true;
    if (!quad_config_covered(s, total_q, force_ft, force_wpq, strict, p)) return false;
    return quad_plan_finish(s, total_q, p);
}

bool quad_plan_bias(const Shape& s, int total_q, bool build_lut, int xf_kind, int force_ft, int force_wpq, bool strict, QuadPlan& p) {
    p = QuadPlan{};
    if (!gemv_quad_supported(s) || s.m_groups >= 1) return false;
    if (xf_kind != 0 && (!build_lut || ((xf_kind & 0xff) != 1 && (xf_kind & 0xff) != 2) || (xf_kind >> 8) != 0)) return false;   // NORM, silu GLU
    p.lutsrc = build_lut ? 1 : 0; p.acc = 1; p.bi = true; p.xf = xf_kind != 0;
    if (build_lut) {
        if (s.K > QUAD_XF_MAX_K || !quad_config_covered(s, total_q, force_ft, force_wpq, strict, p)) return false;
    } else if (!quad_config(s, true, total_q, force_ft, force_wpq, p.ft, p.wpq)) {
        return false;
    }
    return quad_plan_finish(s, total_q, p);
}

// LDS of a capacity-R workgroup: R rows of [4][nst * 64 + 1] uint4 tables + ls / 2, lb / 2 [nst * 32], then the fixed part: partials of the
// eight waves [2 parities][R][8][4 rows][4]
size_t rows_lds_bytes(int K, int R) {
    const int nst = (K / 32 + 63) / 64;
    return (size_t)R * ((size_t)4 * (nst * 64 + 1) * 16 + sizeof(float) * 2 * nst * 32) + sizeof(float) * 2 * R * ROWS_NWV * 16;
}

bool rows_plan(int K, int N, RowsPlan& p) {
    p = RowsPlan{0, 0, 0, 0, 0};
    if (K < 64 || K % 64 != 0 || N < 1) return false;
    for (int R = 8; R >= 2 && !p.r_fit; R >>= 1)
        if (rows_lds_bytes(K, R) <= ROWS_LDS_MAX) p.r_fit = R;
    if (!p.r_fit) return false;
    p.lds_bytes = rows_lds_bytes(K, p.r_fit);
    p.ngroups = (N + p.r_fit - 1) / p.r_fit;
    p.live_last = N - (p.ngroups - 1) * p.r_fit;
    p.cap_last = p.live_last <= 2 ? 2 : p.live_last <= 4 ? 4 : 8;
    return true;
}

bool gemv_rows_supported(const Shape& s) {
    RowsPlan p;
    return gemv_quad_supported(s) && rows_plan(s.K, 2, p);
}

bool rows_launch_plan(const Shape& s, int N, int total_q, RowsLaunchPlan& p) {
    p = RowsLaunchPlan{};
    if (!gemv_rows_supported(s) || N < 1 || !rows_plan(s.K, N, p.rows)) return false;
    const int nst = (s.K / 32 + 63) / 64;
    // waves per quad, by the shape alone (never by N: a row's bits must not depend on the call's N): the fewest of 1 / 2 / 4 that give every
    // CU a workgroup, at most one wave per step
    p.wpq = 1;
    while (p.wpq < 4 && p.wpq * 2 <= nst && (total_q * p.wpq + ROWS_NWV - 1) / ROWS_NWV < 256) p.wpq *= 2;
    const int ipi = ROWS_NWV / p.wpq;
    const int need = (total_q + ipi - 1) / ipi;
    auto add = [&](int R, int n_base, int groups) {
        const size_t shmem = rows_lds_bytes(s.K, R);
        const int occ = shmem * 2 <= ROWS_LDS_MAX ? 2 : 1;             // persistent: at most two workgroups per CU
        p.l[p.nlaunch++] = RowsLaunch{R, n_base, need < 256 * occ ? need : 256 * occ, groups, shmem};
    };
    const RowsPlan& r = p.rows;
    const int full = r.cap_last == r.r_fit ? r.ngroups : r.ngroups - 1;      // groups of capacity r_fit: one launch, blockIdx.y = group
    if (full > 0) add(r.r_fit, 0, full);
    if (full < r.ngroups) add(r.cap_last, full * r.r_fit, 1);
    return true;
}

}  // namespace tmac
