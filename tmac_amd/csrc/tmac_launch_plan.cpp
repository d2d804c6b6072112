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

size_t experts_lds_bytes(int K, int rows) {
    const int nst = (K / 32 + 63) / 64;
    return (size_t)rows * ((size_t)4 * (nst * 64 + 1) * 16 + sizeof(float) * 2 * nst * 32) + sizeof(float) * 2 * EXPERTS_NWV * 4;
}

bool experts_plan(const Shape& s, const int* bank_Mw, int nbanks, int S, int lut_rows, int mode, ExpertsPlan& p) {
    p = ExpertsPlan{false, nullptr, 0, 0, 0, 0};
    auto refuse = [&](const char* why) { p.why = why; return false; };
    if (nbanks < 1 || nbanks > EXPERTS_MAX_BANKS) return refuse("one or two banks per call");
    if (S < 1 || S > EXPERTS_MAX_SLOTS) return refuse("1 to 8 slots per call");
    if (lut_rows != 1 && lut_rows != S) return refuse("lut_rows is 1 (one activation row shared by the slots) or S (one per slot)");
    if (mode != EXPERTS_SLOTS && mode != EXPERTS_COMBINE) return refuse("mode is SLOTS or COMBINE");
    if (mode == EXPERTS_COMBINE && nbanks != 1) return refuse("COMBINE takes one bank");
    if (mode == EXPERTS_COMBINE && lut_rows != S) return refuse("COMBINE takes one activation row per slot (lut_rows = S)");
    int total_q = 0;
    for (int b = 0; b < nbanks; ++b) {
        Shape sb = s;
        sb.Mw = bank_Mw[b];
        if (!gemv_quad_supported(sb)) return refuse("a bank's matrices are outside what k_gemv_quad's layout serves");
        total_q += sb.Mw / 4;
    }
    if (!experts_inst_exists(s.bits, s.m_groups >= 1 ? 2 : 0, mode)) return refuse("unified-scale banks are not served");
    p.lds_bytes = experts_lds_bytes(s.K, lut_rows);
    if (p.lds_bytes > ROWS_LDS_MAX) return refuse("the tables of the call's activation rows do not fit LDS (fewer slots, or a smaller K)");
    const int nst = (s.K / 32 + 63) / 64;
    // waves per quad as rows_launch_plan chooses them, from the banks' quads: a slot's bits must not depend on S, on the mode or on
    // whether x is shared
    p.wpq = 1;
    while (p.wpq < 4 && p.wpq * 2 <= nst && (total_q * p.wpq + EXPERTS_NWV - 1) / EXPERTS_NWV < 256) p.wpq *= 2;
    const int ipi = EXPERTS_NWV / p.wpq;
    p.items = mode == EXPERTS_COMBINE ? total_q : S * total_q;
    const int need = (p.items + ipi - 1) / ipi;
    const int occ = p.lds_bytes * 2 <= ROWS_LDS_MAX ? 2 : 1;      // persistent: at most two workgroups per CU
    p.gx = need < 256 * occ ? need : 256 * occ;
    p.served = true;
    return true;
}

bool experts_rows_sizes(long long N, long long S, long long E, ExpertsRowsSizes& z) {
    z = ExpertsRowsSizes{nullptr, 0, 0};
    if (N < 1) z.why = "N: at least one token";
    else if (S < 1 || S > EXPERTS_MAX_SLOTS) z.why = "S: 1 to 8 slots per token";
    else if (E < 1 || E > EXPERTS_ROWS_MAX_E) z.why = "E: the routing kernel takes 1 to 256 experts";
    else if (N * S > EXPERTS_ROWS_MAX_NS) z.why = "N x S: the routing kernel takes at most 32768 slots";
    if (z.why) return false;
    const long long ns = N * S;
    z.T_max = (int)(ns / 64 + (E < ns ? E : ns));
    z.P = 64 * z.T_max;
    return true;
}

bool experts_router_plan(long long K, long long E, long long S, long long N, bool x_f16, bool w_f16, ExpertsRouterPlan& p) {
    (void)x_f16; (void)w_f16;      // (the two arithmetics walk K alike)
    p = ExpertsRouterPlan{nullptr, 0, 0, 0, 0, 0, 0, 0};
    if (N < 1) p.why = "N: at least one token";
    else if (S < 1 || S > EXPERTS_MAX_SLOTS) p.why = "S: 1 to 8 experts per token";
    else if (E < S) p.why = "E: at least S experts (S <= E)";
    else if (E > ROUTER_MAX_E) p.why = "E: the router takes at most 256 experts";
    else if (N * S > EXPERTS_ROWS_MAX_NS) p.why = "N x S: the router takes at most 32768 slots";
    else if (K < ROUTER_KSTEP || K % ROUTER_KSTEP != 0 || K > (1 << 24)) p.why = "K: a multiple of 64 (up to 2^24)";
    if (p.why) return false;
    const int nsteps = (int)(K / ROUTER_KSTEP);
    p.ctiles = (int)((E + 31) / 32);
    const int want = ROUTER_NWV / p.ctiles < nsteps ? ROUTER_NWV / p.ctiles : nsteps;
    p.steps = (nsteps + want - 1) / want;
    p.slices = (nsteps + p.steps - 1) / p.steps;         // (no empty slice)
    p.waves = p.ctiles * p.slices;
    p.e_pad = 32 * p.ctiles;
    p.gx = (int)((N + ROUTER_TOKENS - 1) / ROUTER_TOKENS);
    p.lds_bytes = sizeof(float) * p.slices * ROUTER_TOKENS * p.e_pad;
    if (p.lds_bytes > ROWS_LDS_MAX) { p.why = "the slices' partial tiles do not fit LDS"; return false; }
    return true;
}

bool experts_gemm_plan(const Shape& s, const int* bank_Mw, int nbanks, long long N, long long S, long long E, long long P, ExpertsGemmPlan& p) {
    p = ExpertsGemmPlan{nullptr, 0, 0, {0, 0}, 0};
    auto refuse = [&](const char* why) { p.why = why; return false; };
    if (nbanks < 1 || nbanks > EXPERTS_MAX_BANKS) return refuse("one or two banks per call");
    // the per-group-scale branch of gemm_planes_supported (tmac_gemm2.hip), which this file cannot call: QUAD layout, 1-4 bits, act groups
    // of 64, weight groups of 64 x 2^n that divide K
    const int apg = s.gs / 64;
    if (s.lay != 2 || s.bits < 1 || s.bits > 4 || s.K < 64 || s.K % 64 != 0 || s.m_groups >= 1 || s.ags != 64 || s.gs < 64 || s.gs % 64 != 0 ||
        s.K % s.gs != 0 || (apg & (apg - 1)) != 0)
        return refuse("outside what k_gemm_planes' per-group arithmetic serves (QUAD layout, 1-4 bits, K a multiple of 64, act groups of 64, group sizes 64 x 2^n, per-group scales)");
    ExpertsRowsSizes z;
    if (!experts_rows_sizes(N, S, E, z)) return refuse(z.why);
    if (P != z.P) return refuse("P is not 64 x T_max of (N, S, E): the outputs and the routing belong to another call shape");
    if ((size_t)2 * s.K * (size_t)P >= ((size_t)1 << 31)) return refuse("the position image reaches 2 GB (32-bit buffer offsets): fewer tokens per call");
    int gx = 0;
    for (int b = 0; b < nbanks; ++b) {
        const int Mw = bank_Mw[b];
        if (Mw < 4 || Mw % 4 != 0) return refuse("a bank's Mw must be a multiple of 4");
        if ((size_t)(Mw / 4) * ((s.K / 32 + 63) / 64) * s.bits * 1024 >= ((size_t)1 << 31)) return refuse("an expert's matrix reaches 2 GB (32-bit buffer offsets)");
        const int tiles = (Mw + 63) / 64;
        gx += (tiles + EXPERTS_GEMM_NWV - 1) / EXPERTS_GEMM_NWV;
        p.wg_end[b] = gx;
    }
    p.gx = gx; p.gy = z.T_max;
    p.lds_bytes = EXPERTS_GEMM_LDS_BYTES;
    return true;
}

}  // namespace tmac
