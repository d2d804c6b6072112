// tmac_launch.cpp — the entry points of the kernels that are built one translation unit per weight width (k_gemv_quad: and scale dtype;
// k_gemv_rows): check the call, plan it (tmac_launch_plan.h), hand the plan to the unit that holds the call's kernels.
#include "tmac_kernels.h"
#include "tmac_chain.h"
#include "tmac_select.h"

namespace tmac {

// a: precomputed.  The fp16-scale units hold the per-group-scale kernels alone: a unified scale keeps its dtype a run-time flag.
template <class Args>
static hipError_t quad_unit(const Args& a, const QuadPlan& p, int N, hipStream_t st) {
    return sel_int<1, 2, 3, 4>(a.s.bits, [&](auto BITS) { return sel_bool(a.sc_f16 && a.s.m_groups < 1, [&](auto SCF16) {
        return launch_gemv_quad_unit<BITS.value, SCF16.value>(a, p, N, st);
    }); });
}

// launch_gemv_quad, one overload per argument block: what the block's instantiations take (ok), its planner, then the unit.
// a.m[i].nb_end must hold cumulative QUAD counts.  ft / wpq: 0 = heuristic (A/B knobs)
template <class Args, class Planner>
static hipError_t quad_launch(const Args& a_in, bool ok, int N, hipStream_t st, Planner plan) {
    QuadPlan p;
    if (a_in.nmat < 1 || a_in.nmat > 4 || !ok || !plan(a_in.m[a_in.nmat - 1].nb_end, p)) return hipErrorInvalidValue;
    Args a = a_in;
    fused_precompute(a);
    return quad_unit(a, p, N, st);
}
hipError_t launch_gemv_quad(const FusedArgs& a, int N, bool build_lut, int ft, int wpq, bool, hipStream_t st) {
    return quad_launch(a, true, N, st, [&](int total_q, QuadPlan& p) { return quad_plan(a.s, total_q, build_lut, a.dump != nullptr, a.acc_mfma != 0, ft, wpq, p); });
}

static bool xf_args_bad(const FusedXfArgs& a) {
    const int kind = a.xf_kind & 0xff, gate = a.xf_kind >> 8;
    if (kind != 1 && kind != 2 && kind != 4) return true;
    if (gate < 0 || gate > 2 || (kind == 1 && gate != 0)) return true;      // silu, relu^2, tanh-GELU (tmac_quad_core.h XF_GATE_*); NORM has no gate
    return kind == 4 && (!a.in2 || !a.gamma);
}
hipError_t launch_gemv_quad(const FusedXfArgs& a, int N, bool build_lut, int ft, int wpq, bool strict, hipStream_t st) {
    return quad_launch(a, N == 1 && build_lut && a.acc_mfma && !a.dump && !xf_args_bad(a), 1, st,
                       [&](int total_q, QuadPlan& p) { return quad_plan_xf(a.s, total_q, a.xf_kind, ft, wpq, strict, p); });
}
hipError_t launch_gemv_quad(const FusedPermArgs& a, int N, bool build_lut, int ft, int wpq, bool strict, hipStream_t st) {
    return quad_launch(a, N == 1 && build_lut && a.acc_mfma && !a.dump && !a.lut_tap && a.perm, 1, st,
                       [&](int total_q, QuadPlan& p) { return quad_plan_perm(a.s, total_q, ft, wpq, strict, p); });
}

// the bias blocks: per-group scales, MFMA accumulate, no tap of any kind; at least one matrix with a bias (the others: null)
template <class Args>
static bool bias_args_ok(const Args& a) {
    bool any = false;
    for (int i = 0; i < a.nmat && i < 4; ++i) any = any || a.bias[i] != nullptr;
    return any && a.acc_mfma && !a.dump && !a.lut_tap && !a.stamps && a.s.m_groups < 1;
}
hipError_t launch_gemv_quad(const FusedBiasArgs& a, int N, bool build_lut, int ft, int wpq, bool strict, hipStream_t st) {
    return quad_launch(a, N >= 1 && bias_args_ok(a), N, st,
                       [&](int total_q, QuadPlan& p) { return quad_plan_bias(a.s, total_q, build_lut, 0, ft, wpq, strict, p); });
}
hipError_t launch_gemv_quad(const FusedXfBiasArgs& a, int N, bool build_lut, int ft, int wpq, bool strict, hipStream_t st) {
    return quad_launch(a, N == 1 && build_lut && bias_args_ok(a) && !xf_args_bad(a), 1, st,
                       [&](int total_q, QuadPlan& p) { return quad_plan_bias(a.s, total_q, true, a.xf_kind, ft, wpq, strict, p); });
}

// *launches (optional) grows by the number of k_gemv_rows launches made
hipError_t launch_gemv_rows(const RowsArgs& a_in, hipStream_t st, int* launches) {
    RowsArgs a = a_in;
    RowsLaunchPlan p;
    if (a.nmat < 1 || a.nmat > 4 || (a.tap && a.nmat != 1) || !rows_launch_plan(a.s, a.N, a.m[a.nmat - 1].nb_end, p)) return hipErrorInvalidValue;
    const Shape& s = a.s;
    a.nu = s.K / 32; a.nst = (a.nu + 63) / 64; a.tstride = ((a.nu + 15) & ~15) + 1;
    a.G = s.K / s.ags; a.nsg = s.gs > 0 && s.m_groups < 1 ? s.K / s.gs : 1;
    a.gs_shift = 0;
    if (s.gs > 0) for (int g = s.gs / 32; g > 1; g >>= 1) ++a.gs_shift;
    if (s.m_groups >= 1) a.gs_shift = 2;
    for (int i = 0; i < a.nmat; ++i) {
        // fragment offsets are 32-bit buffer offsets
        if ((size_t)((a.m[i].Mw + 3) / 4) * a.nst * s.bits * 1024 >= ((size_t)1 << 31)) return hipErrorInvalidValue;
    }
    a.wpq = p.wpq;
    for (int i = 0; i < p.nlaunch; ++i) {
        a.n_base = p.l[i].n_base; a.rows_per_group = p.l[i].R;
        const hipError_t e = sel_int<1, 2, 3, 4>(s.bits, [&](auto BITS) { return launch_gemv_rows_unit<decltype(BITS)::value>(a, p.l[i], st); });
        if (e != hipSuccess) return e;
        if (launches) ++*launches;
    }
    return hipSuccess;
}

// ---- the decode chain and stream mode (tmac_chain.h): units by weight width and G2 / by form and G2 ----
hipError_t launch_decode_chain(const ChainArgs& a, int bits, bool zp, bool sc_f16, int sm, bool g2, int grid, size_t lds_bytes, hipStream_t st, int* resident) {
    return sel_int<1, 2, 3, 4>(bits, [&](auto BITS) { return sel_bool(g2, [&](auto G2) {
        return launch_decode_chain_unit<decltype(BITS)::value, decltype(G2)::value>(a, zp, sc_f16, sm, grid, lds_bytes, st, resident);
    }); });
}
hipError_t launch_gemv_stream(const StreamArgs& a, int bits, bool zp, bool sc_f16, int sm, bool qw, bool g2, int grid, size_t lds_bytes, hipStream_t st) {
    if (a.nops < 1 || grid < 1 || a.nsplit < 1 || a.nsplit > 4 || (sm != 0 && sm != 2) || (g2 && sm != 0)) return hipErrorInvalidValue;
    return sel_bool(qw, [&](auto QW) { return sel_bool(g2, [&](auto G2) {
        return launch_gemv_stream_unit<decltype(QW)::value, decltype(G2)::value>(a, bits, zp, sc_f16, sm, grid, lds_bytes, st);
    }); });
}

}  // namespace tmac
