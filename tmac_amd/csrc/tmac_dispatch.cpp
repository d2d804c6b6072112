// tmac_dispatch.cpp — qgemm_lut dispatch: which kernel serves a call (decode GEMV variants, the N > 1 GEMMs, the fused
// LUT-build + GEMV entry point and its prefill route) and the parity taps around them.  A call is planned (plan_split /
// plan_fused name the kernel: enum Route), then launched.  A fused call is one value (FusedCall, tmac_host.h): its doors share named
// checks, one planner call (plan_call) and one launch site for k_gemv_quad (launch_quad).
#include "tmac_host.h"

using namespace tmac_host;

// ---- the plan: what runs -------------------------------------------------------------------------------------------------
enum Route {
    R_GEMM_PLANES,   // k_gemm_planes / k_gemm_planes_us on the workspace's LUT image
    R_GEMM_ONEHOT,   // k_gemm_onehot on the half-table image
    R_GEMV_QUAD,     // k_gemv_quad (QUAD layout)
    R_GEMV_ROWS,     // k_gemv_rows (QUAD layout): 2-8 activation rows per weight pass, tables copied from the half-table image
    R_GEMV_FUSED,    // k_gemv_fused (row-block layout)
    R_GEMV_LO,       // k_gemv_lo (two-kernel path; v_mqsad or SDWA accumulate by the variant knob)
    R_REF_LAYOUT,    // k_gemv_ref_layout on the reference blobs
    R_ROW_LOOP       // fused entry point's last resort: one LUT build, then tmac_hip_qgemm_dev (plan_split) per matrix
};
static const char* const ROUTE_NAMES[] = {"k_gemm_planes", "k_gemm_onehot", "k_gemv_quad", "k_gemv_rows", "k_gemv_fused", "k_gemv_lo", "k_gemv_ref_layout", "the row loop"};
struct Plan {
    Route route;
    LutBuild lut;      // the LUT the fused entry point builds before the planned kernel (tmac_lut_held.h; the split entry points find theirs in the workspace)
    int32_t err;       // TMAC_HIP_OK, or the call is refused: fail(err, msg, mat)
    const char* msg;   // (may name the offending matrix: %d)
    int mat;
};
static Plan planned(Route r, LutBuild lut = LB_NONE) { return Plan{r, lut, TMAC_HIP_OK, nullptr, 0}; }
static Plan refused(int32_t code, const char* msg, int mat = 0) { return Plan{R_ROW_LOOP, LB_NONE, code, msg, mat}; }
// tmac_hip_debug_route_stats: one count per planned route at the site that launches it (the row loop counts itself, then each matrix
// counts the route plan_split gave it)
static void count_route(Route r) { ++g_knobs.route_launches[r]; }

// ---- predicates of the plan ------------------------------------------------------------------------------------------------
// matrices that can be served from one LUT | by one kernel instantiation
static bool same_lut(const tmac_hip_weights* a, const tmac_hip_weights* b) { return a->s.K == b->s.K && a->s.ags == b->s.ags; }
static bool same_quant(const tmac_hip_weights* a, const tmac_hip_weights* b) {
    return a->s.bits == b->s.bits && a->s.gs == b->s.gs && a->s.zero_point == b->s.zero_point && a->s.m_groups == b->s.m_groups &&
           a->sc_dtype == b->sc_dtype;
}
// ... what a call that breaks either is told (plan_fused, one_lut_check)
static const char* const ONE_LUT_MSG = "matrices fused in one launch must share K, bits and quantisation config";
// GEMM or row loop for N activation rows on matrices with total_Mw output rows?  An explicitly set threshold
// (tmac_hip_set_gemm_min_n) is taken literally.  Otherwise: the measured crossover per launch where k_gemm_planes covers the
// configuration (planes_pays), and k_gemm_onehot only from 32 rows on with a grid that fills the chip (onehot_pays: with fewer
// than 128 workgroups of 128 bit-plane rows the row loop is faster up to 64 rows: 4096 x 11008 at N = 32: 88 us against 152 us).
static bool planes_covers(const Shape& s) { return g_knobs.gemm_kernel != 1 && layout_of(s) == L_QUAD && gemm_planes_supported(s); }
static bool onehot_pays(const Shape& s, long total_Mw, int N) {
    return N >= gemm_min_rows(32) && (g_knobs.gemm_min_n != 32 || N >= 64 || (total_Mw * s.bits + 127) / 128 >= 128);
}
static int planes_crossover(const Shape& s, long total_Mw, int N) {
    // From how many activation rows on k_gemm_planes beats the GEMV kernel looped over the rows: measured on MI355X, llama-2-7B shapes,
    // 1- to 4-bit weights (tools/bench_small_n.py, profiles/r03_small_n.txt).  The row loop costs ~3 us + N x (0.7 us + 0.155 us per MB
    // of weights + 0.2 us per 1000 of K beyond 4096); the GEMM (6 + 14 K / 4096) us per wave of 64 x 64 tiles (x 1.18 for 3- / 4-bit
    // operand rows) whatever N <= 64 is.  Crossovers (W2): o 14, q/k/v 7, gate/up 7, down 9 rows; the fixed 12 rows of round 2 -- which
    // the fused entry point applied on top of a fixed 32 -- left up to 2 x on the table for 7-31 rows.  5 % margin for the row loop.
    const double mb = (double)total_Mw * s.K * s.bits / 8e6, tiles = (double)((total_Mw + 63) / 64) * ((N + 63) / 64);
    const double waves = tiles <= 256.0 ? 1.0 : s.bits == 4 ? (double)(((long)tiles + 255) / 256) : (s.bits == 3 ? 0.45 : 0.25) + tiles / 256.0;
    const double tp = (6.0 + 14.0 * s.K / 4096.0) * waves * (s.bits >= 3 ? 1.18 : 1.0);
    const double c1 = 0.7 + 0.155 * mb + 0.2 * (s.K > 4096 ? (s.K - 4096) / 1000.0 : 0.0);
    const int nmin = (int)((1.05 * tp - 3.0) / c1 + 0.999);
    return nmin < 4 ? 4 : nmin > 16 ? 16 : nmin;
}
static bool planes_pays(const Shape& s, long total_Mw, int N) { return N >= gemm_min_rows(planes_crossover(s, total_Mw, N)); }
// the fused entry point builds whatever LUT form the chosen kernel wants, so one question decides
static bool gemm_pays(const Shape& s, long total_Mw, int N) { return planes_covers(s) ? planes_pays(s, total_Mw, N) : onehot_pays(s, total_Mw, N); }
static bool planes_ok(const tmac_hip_weights* w) {
    return planes_covers(w->s) && w->tiled_ok && !w->fa && w->w_bytes < ((size_t)1 << 31);
}
// Where auto mode hands an N >= 2 call below the GEMM crossover to k_gemv_rows instead of the row loop (k_gemv_quad, grid.y = N).
// The rule: only where the rows kernel's column of profiles/r09_small_n.txt beats the DEFAULT column of profiles/r09_small_n_parent.txt
// (the parent commit, same GPU session) by more than 5 %, the margin planes_crossover gives the incumbent.  Measured (llama-2-7B shapes,
// W2 and W4, N = 2 ... 16): no shape class and N clears it -- rows / parent default is 2.1 on o and qkv, 1.4-1.5 on gate/up, 1.02-1.27 on
// down -- so auto is the routing without the kernel everywhere and planes_crossover keeps its fit against the row loop, the cheaper of the
// two at every measured point.  Rows-kernel cost shape (W2 fit, not a bar): us ~ 5 + groups x (0.155 per MB of weights + live rows x
// (1.3 + 0.16 per MB)); the per-row term is what the next round has to cut.
static bool rows_auto(const Shape& s, long total_Mw, int N) {
    (void)s; (void)total_Mw; (void)N;
    return false;
}
// k_gemv_rows: can it serve these weights at all | does auto mode want it (tmac_hip_debug_rows_kernel: 1 never, 2 always)
static bool rows_covers(const tmac_hip_weights* w) {
    return (g_knobs.variant == V_AUTO || g_knobs.variant == V_QUAD) && layout_of(w->s) == L_QUAD && w->tiled_ok && !w->fa && gemv_rows_supported(w->s);
}
static bool rows_pays(const Shape& s, long total_Mw, int N) {
    if (g_knobs.rows_kernel != 0) return g_knobs.rows_kernel == 2;
    return rows_auto(s, total_Mw, N);
}

// ---- the two planners ------------------------------------------------------------------------------------------------------
// They read g_knobs and their arguments, take no lock, allocate nothing and launch nothing.  Today's routing, quirks included
// (none of them is this file's to fix):
//  * Split entry points (tmac_hip_qgemm_dev, the host-pointer C-ABI, the row loop below).  The weights' device layout decides which
//    tiled kernel can run; the variant knob only picks V_REF_LAYOUT and the accumulate of k_gemv_lo.  Weights without a tiled kernel
//    go to the reference layout whatever the knob says.  k_gemm_planes only when the workspace holds a valid LUT image of the kind
//    the shape wants: tmac_hip_preprocessor_dev builds it from PLANES_MIN_N rows on (it does not know the matrix), while the
//    crossover applied here is the measured one of the matrix -- between the two the image is built and not used, or wanted and not
//    there.  Without the image only k_gemm_onehot's own, later crossover counts: below it the row loop is the faster kernel.  The
//    image counts only while the workspace holds it (LutHeld::serves_image): every build or write of the LUT starts from a workspace
//    that holds nothing.
//  * A tap bypasses k_gemm_planes on the split entry point, but not k_gemm_onehot, which has a per-plane tap of its own.  On the
//    fused entry point a tap (dump / lut_tap) bypasses both GEMMs -- and, in fused_impl, recording and the deferred queue.
//  * Fast-aggregation weights are accepted on V_REF_LAYOUT, V_LO_MQSAD and V_LO_SDWA only (registration puts them in the LO layout,
//    so the refusal cannot be reached with weights this library registered).
//  * Fused entry point, N >= 2.  The GEMM family is entered when every matrix is covered by one of the two GEMMs and gemm_pays says
//    so for the FIRST matrix's shape over the rows of all: the planes crossover whenever that shape is coverable, even when
//    planes_ok then fails for the weights (fast aggregation, 2 GB) or the matrices differ, and k_gemm_onehot runs below its own
//    crossover.  1- and 3-bit matrices that k_gemm_planes cannot take, a mix of configurations and V_REF_LAYOUT go to the row loop,
//    where each matrix is planned again from the workspace's state: after LB_ALL that may be a GEMM after all, after
//    LB_HALF_TABLES k_gemv_quad or k_gemm_onehot (the half-table build invalidates the image: none is found, whatever ran before).
//  * The K > PAIRS_ROW_MAX_K limit applies to the row-wise image: unified-scale matrices beyond it get k_gemm_onehot on the LUT of
//    the one-workgroup-per-act-group build.
//  * image_fits: the LUT image of the stream's workspace, which has the row stride of the largest N the stream has seen, stays below
//    2 GB.  fused_impl plans before the workspace exists and assumes it does; fused_prefill plans again where it does not.
//  * N = 1, a tap, or a GEMM that does not pay: one fused GEMV launch; the matrices must share layout, K and quantisation config.
//  * k_gemv_rows (R_GEMV_ROWS; tmac_hip_debug_rows_kernel: 0 auto, 1 off = everything above bit for bit, 2 forced).  It stands where
//    k_gemv_quad would be launched with grid.y = N: N >= 2, no tap, neither GEMM chosen, QUAD-layout weights it covers (rows_covers: what
//    gemv_quad_supported accepts, variant 0 or 6, no fast aggregation), and rows_pays says so (auto: rows_auto, the measured rule; forced:
//    always).  Forced mode is asked BEFORE the GEMM thresholds: every N >= 2 call the kernel covers takes it.
//    Split entry points: the workspace always holds the half-table image (tmac_hip_preprocessor_dev and tmac_hip_workspace_write fill
//    qlut_lds), so the route needs nothing else.  Fused entry point: all matrices in the QUAD layout with same_lut and same_quant
//    (rows_fused_ok) -> planned(R_GEMV_ROWS, LB_HALF_TABLES): the pair build into the stream's library workspace (fused_prefill), then ONE
//    k_gemv_rows call over all matrices.  Unified-scale matrices with K > PAIRS_ROW_MAX_K keep the route above (the row-wise pair build
//    does not reach them).  Taps (tmac_hip_qgemm_partial_sums, tmac_hip_qgemm_fused_partial_sums) never take it; its own tap is
//    tmac_hip_debug_rows_comb_sums.  Recording and deferral sit in front of the planner (fused_impl) and do not know the route.
//  * A transformed call of N >= 2 rows (tmac_hip_qgemm_fused_xf_rows_dev) takes plan_fused's answer with two rules of its own
//    (xf_rows_plan, at the fused entry point): R_GEMV_QUAD becomes R_ROW_LOOP behind LB_HALF_TABLES -- the transform lives in the N > 1
//    LUT builders, so the image is built once and each matrix is planned again by plan_split -- and a plan that needs LB_ALL is refused.
//    Routing of untransformed calls is untouched.
// image_ok: the workspace holds a valid LUT image of the kind the shape wants for N rows, addressable by k_gemm_planes (plan_split: of the
// call's workspace; bias_routes_check asks both ways before a workspace exists)
static Plan plan_split_on(const tmac_hip_weights* w, bool image_ok, int N, bool tap) {
    Route r = R_REF_LAYOUT;
    if (g_knobs.variant != V_REF_LAYOUT && w->tiled_ok)
        r = layout_of(w->s) == L_QUAD ? R_GEMV_QUAD : layout_of(w->s) == L_ROWBLOCK ? R_GEMV_FUSED : R_GEMV_LO;
    if (w->fa && r != R_REF_LAYOUT && r != R_GEMV_LO) return refused(TMAC_HIP_E_NOMATCH, "fast-aggregation weights run on the two-kernel path only");
    if (r == R_REF_LAYOUT && !w->A_ref)
        return refused(TMAC_HIP_E_NOMATCH, "reference-layout blobs were not kept for these weights (register them with variant 3 selected)");
    if (r != R_GEMV_QUAD && r != R_GEMV_FUSED) return planned(r);
    const bool rows = r == R_GEMV_QUAD && N >= 2 && !tap && g_knobs.rows_kernel != 1 && rows_covers(w);
    if (rows && g_knobs.rows_kernel == 2) return planned(R_GEMV_ROWS);
    if (!tap && image_ok && planes_ok(w) && planes_pays(w->s, w->s.Mw, N))
        return planned(R_GEMM_PLANES);
    if (onehot_pays(w->s, w->s.Mw, N) && gemm_onehot_supported(w->s)) return planned(R_GEMM_ONEHOT);
    if (rows && rows_pays(w->s, w->s.Mw, N)) return planned(R_GEMV_ROWS);
    return planned(r);
}
static Plan plan_split(const tmac_hip_weights* w, const tmac_hip_workspace* ws, int N, bool tap) {
    return plan_split_on(w, ws->held.serves_image(image_kind_for(w->s), w->s.K, N) && ws->image_fits(w->s.K), N, tap);
}

// every matrix in the QUAD layout, one LUT, one kernel instantiation, and a pair build that covers the LUT
static bool rows_fused_ok(const tmac_hip_weights* const* wl, void* const* C_list, int nmat) {
    long rows = 0;
    for (int i = 0; i < nmat; ++i) {
        const tmac_hip_weights* w = wl[i];
        if (!w || !C_list[i] || !rows_covers(w) || !same_lut(w, wl[0]) || !same_quant(w, wl[0])) return false;
        rows += w->s.Mw;
    }
    const Shape& s0 = wl[0]->s;
    return rows > 0 && !(s0.m_groups >= 1 && s0.K > PAIRS_ROW_MAX_K);
}
static Plan plan_fused(const tmac_hip_weights* const* wl, void* const* C_list, int nmat, int N, bool tap, bool image_fits = true) {
    const bool rows = N >= 2 && !tap && g_knobs.rows_kernel != 1 && rows_fused_ok(wl, C_list, nmat);
    if (rows && g_knobs.rows_kernel == 2) return planned(R_GEMV_ROWS, LB_HALF_TABLES);
    if (g_knobs.gemm_min_n > 0 && N >= 2 && !tap) {       // (gemm_pays applies the threshold: a set one, or the measured crossover)
        bool ok = true, quant = true, all_planes = true, all_onehot = true, all_quad = true;
        long rows = 0;
        for (int i = 0; i < nmat && ok; ++i) {
            const tmac_hip_weights* w = wl[i];
            ok = w && C_list[i] && (gemm_onehot_supported(w->s) || planes_ok(w)) && same_lut(w, wl[0]);
            if (!ok) break;
            rows += w->s.Mw;
            quant = quant && same_quant(w, wl[0]);
            all_planes = all_planes && planes_ok(w);
            all_onehot = all_onehot && gemm_onehot_supported(w->s);
            all_quad = all_quad && layout_of(w->s) == L_QUAD && w->tiled_ok && !w->fa;
        }
        if (ok && gemm_pays(wl[0]->s, rows, N)) {
            const Shape& s0 = wl[0]->s;
            const bool tiled = g_knobs.variant != V_REF_LAYOUT;
            // the plane-combined GEMM reads its own LUT image only: one build, one launch for all matrices
            if (tiled && image_fits && all_planes && quant && !(s0.m_groups >= 1 && s0.K > PAIRS_ROW_MAX_K)) return planned(R_GEMM_PLANES, LB_IMAGE);
            const LutBuild lut = tiled && all_onehot && (s0.ags == 64 || (s0.ags == s0.K && s0.K <= PAIRS_ROW_MAX_K)) ? LB_HALF_TABLES : LB_ALL;
            if (tiled && all_onehot && quant && all_quad) return planned(R_GEMM_ONEHOT, lut);   // q/k/v or gate/up: one launch fills the chip
            return planned(R_ROW_LOOP, lut);
        }
    }
    for (int i = 0; i < nmat; ++i) {
        const tmac_hip_weights* w = wl[i];
        if (!w || !C_list[i]) return refused(TMAC_HIP_E_ARG, "null matrix or output");
        if (layout_of(w->s) == L_LO || !w->tiled_ok || layout_of(w->s) != layout_of(wl[0]->s))
            return refused(TMAC_HIP_E_NOMATCH, "matrix %d is not registered in the fused layout", i);
        if (!same_lut(w, wl[0]) || !same_quant(w, wl[0])) return refused(TMAC_HIP_E_ARG, ONE_LUT_MSG);
    }
    if (rows) {
        long total = 0;
        for (int i = 0; i < nmat; ++i) total += wl[i]->s.Mw;
        if (rows_pays(wl[0]->s, total, N)) return planned(R_GEMV_ROWS, LB_HALF_TABLES);
    }
    return planned(layout_of(wl[0]->s) == L_QUAD ? R_GEMV_QUAD : R_GEMV_FUSED);
}

// ---- one plan per call -----------------------------------------------------------------------------------------------------
// A transformed call of N >= 2 rows (tmac_hip_qgemm_fused_xf_rows_dev) runs on a plan of plan_fused with two rules of its own: where the
// planner answers R_GEMV_QUAD (k_gemv_quad with grid.y = N, each workgroup building its row's LUT) the call takes R_ROW_LOOP behind
// LB_HALF_TABLES -- the transform sits in the pair build, k_gemv_quad copies the image (LUTSRC == 0) -- and a plan that needs LB_ALL (the
// three-layout build has no XF instantiation) is refused.  A call on act-order handles takes the same two (its gather sits where the
// transform would).
static Plan xf_rows_plan(Plan p) {
    if (p.err) return p;
    if (p.route == R_GEMV_QUAD) return planned(R_ROW_LOOP, LB_HALF_TABLES);
    if (p.lut != LB_IMAGE && p.lut != LB_HALF_TABLES)
        return refused(TMAC_HIP_E_NOMATCH, "a transformed call of several rows needs the LUT image or the half-table image alone; this plan builds every layout");
    return p;
}
// The plan of a fused call, for every door, both debug twins and fused_prefill's re-plan.  in_build: the call carries a vector transform
// or a K permutation, which for N >= 2 rows lives in the LUT build (xf_rows_plan); image_fits: see the planners.
static Plan plan_call(const FusedCall& c, bool tap, bool in_build = false, bool image_fits = true) {
    const Plan p = plan_fused(c.wl, c.C, c.nmat, c.N, tap, image_fits);
    return in_build && c.N >= 2 ? xf_rows_plan(p) : p;
}
int32_t tmac_host::fused_check(const FusedCall& c) {
    const Plan p = plan_call(c, false);
    return p.err ? fail(p.err, p.msg, p.mat) : TMAC_HIP_OK;
}

// ---- argument blocks of the planned kernels --------------------------------------------------------------------------------
// the split entry point's matrix (and the taps') as a one-matrix call for the launch helpers below
static FusedCall one_matrix(const tmac_hip_weights* const* w, void* const* C, tmac_dtype_t out, int N, hipStream_t st) {
    return FusedCall{w, 1, nullptr, TMAC_F32, C, out, N, st};
}
// does a matrix of the call carry a bias (tmac_hip_weights_set_bias_dev)?  One fused call may mix biased and plain matrices.
static bool any_bias(const FusedCall& c) {
    for (int i = 0; c.wl && i < c.nmat; ++i)
        if (c.wl[i] && c.wl[i]->bias) return true;
    return false;
}
static void fill_gemm_mats(GemmMat* m, const FusedCall& c) {
    for (int i = 0; i < c.nmat; ++i) { m[i].W = c.wl[i]->W; m[i].SC = c.wl[i]->SC; m[i].C = c.C[i]; m[i].Mw = c.wl[i]->s.Mw; }
}
int tmac_host::fill_fused_args(FusedArgs& fa, const FusedCall& c) {
    memset(&fa, 0, sizeof(fa));
    fa.nmat = c.nmat; fa.s = c.s0();
    const bool quad = layout_of(fa.s) == L_QUAD;
    int nb = 0;
    for (int i = 0; i < c.nmat; ++i) {
        const Shape& a = c.wl[i]->s;
        nb += quad ? a.nquads() : a.nb();
        fa.m[i].W = (const uint4*)c.wl[i]->W; fa.m[i].SC = c.wl[i]->SC; fa.m[i].C = c.C[i]; fa.m[i].Mw = a.Mw; fa.m[i].nb_end = nb;
    }
    fa.B = c.B; fa.act_f16 = c.act_f16();
    fa.sc_f16 = c.wl[0]->sc_dtype == F16; fa.out_f16 = c.out_f16();
    fa.acc_mfma = quad ? (g_knobs.variant != V_QUAD_MQSAD) : (g_knobs.variant == V_FUSED_MFMA);
    return nb;
}
static int32_t fused_gemv_rc(hipError_t e, const char* nomatch = "no fused GEMV kernel for this configuration", const char* what = "fused gemv") {
    if (e == hipErrorInvalidValue) return fail(TMAC_HIP_E_NOMATCH, "%s", nomatch);
    if (e != hipSuccess) return fail(TMAC_HIP_E_RUNTIME, "%s launch: %s", what, hipGetErrorString(e));
    return TMAC_HIP_OK;
}

// one-hot MFMA GEMM over 1..4 matrices that share K, the quantisation config (checked by the planners) and the LUT in ws
static int32_t gemm_multi(const FusedCall& c, const tmac_hip_workspace* ws, int32_t* dump) {
    GemmArgs ga;
    memset(&ga, 0, sizeof(ga));
    ga.s = c.s0(); ga.nmat = c.nmat;
    fill_gemm_mats(ga.m, c);
    ga.sc_f16 = c.wl[0]->sc_dtype == F16; ga.out_f16 = c.out_f16();
    ga.qlut_lds = ws->qlut_lds; ga.tstride = (((ga.s.K / 32) + 15) & ~15) + 1; ga.lut_scales = ws->lut_scales; ga.lut_biases = ws->lut_biases;
    ga.dump = dump; ga.N = c.N;
    hipError_t e = launch_gemm_onehot(ga, c.st);
    if (e != hipSuccess) return fail(TMAC_HIP_E_RUNTIME, "one-hot gemm launch: %s", hipGetErrorString(e));
    return TMAC_HIP_OK;
}

// k_gemm_planes over up to 4 matrices that share K and the quantisation config; the workspace holds the LUT image
// (a call with a biased matrix: the bias instantiations, never with the tap)
static int32_t planes_multi(const FusedCall& c, const tmac_hip_workspace* ws, int32_t* comb_dump) {
    Gemm2BiasArgs ga;
    memset(&ga, 0, sizeof(ga));
    for (int i = 0; i < c.nmat; ++i) ga.bias[i] = c.wl[i]->bias;
    ga.s = c.s0(); ga.nmat = c.nmat;
    fill_gemm_mats(ga.m, c);
    ga.sc_f16 = c.wl[0]->sc_dtype == F16; ga.out_f16 = c.out_f16();
    ga.bimg = (const uint4*)ws->gimg; ga.colv = ws->gcol; ga.Npad = ws->gNpad; ga.N = c.N; ga.dump = comb_dump;
    ga.stamps = g_knobs.gemm_stamps;
    ga.form = g_knobs.gemm_kernel == 2 ? 1 : g_knobs.gemm_kernel == 3 ? 2 : 0;
    if (comb_dump && any_bias(c)) return fail(TMAC_HIP_E_ARG, "a parity tap on a handle that carries a bias is not served");
    hipError_t e = any_bias(c) ? launch_gemm_planes(ga, c.st) : launch_gemm_planes(static_cast<const Gemm2Args&>(ga), c.st);
    if (e == hipErrorInvalidValue) return fail(TMAC_HIP_E_NOMATCH, "plane-combined gemm: configuration or sizes not covered (LUT image and matrices must stay below 2 GB)");
    if (e != hipSuccess) return fail(TMAC_HIP_E_RUNTIME, "plane-combined gemm launch: %s", hipGetErrorString(e));
    return TMAC_HIP_OK;
}

// k_gemv_rows over up to 4 matrices that share K and the quantisation config; the workspace holds the half-table image of N rows
static int32_t rows_multi(const FusedCall& c, const tmac_hip_workspace* ws, int32_t* tap) {
    FusedArgs fa;
    fill_fused_args(fa, c);
    RowsArgs ra;
    memset(&ra, 0, sizeof(ra));
    for (int i = 0; i < c.nmat; ++i) ra.m[i] = fa.m[i];
    ra.nmat = c.nmat; ra.s = fa.s; ra.sc_f16 = fa.sc_f16; ra.out_f16 = fa.out_f16;
    ra.qlut_lds = ws->qlut_lds; ra.lut_scales = ws->lut_scales; ra.lut_biases = ws->lut_biases;
    ra.tap = tap; ra.N = c.N;
    int launches = 0;
    const hipError_t e = launch_gemv_rows(ra, c.st, &launches);
    g_knobs.rows_launches += (uint64_t)launches;
    if (e == hipErrorInvalidValue) return fail(TMAC_HIP_E_NOMATCH, "rows kernel: configuration or sizes not covered (matrices must stay below 2 GB)");
    if (e != hipSuccess) return fail(TMAC_HIP_E_RUNTIME, "rows kernel launch: %s", hipGetErrorString(e));
    return TMAC_HIP_OK;
}

// ---- act-order handles (tmac_kperm.h) ------------------------------------------------------------------------------------------
// A handle that carries a K permutation holds W[:, perm]: every LUT it meets must have been built from x[perm].  The fused entry point
// gathers in its LUT build (k_gemv_quad's GA instantiations for N = 1, the gathered pair build / LUT image for N >= 2); the split entry
// point checks the workspace's record of the permutation its LUT was built through; everything else refuses such handles.
static const KPermData* perm_of(const tmac_hip_weights* w) { return w ? w->kperm.get() : nullptr; }
static uint64_t perm_id_of(const tmac_hip_weights* w) { return w && w->kperm ? w->kperm->h.id : 0; }
// 0: no matrix carries a permutation | 1: all carry the same one (tmac_kperm.h: one object, or equal contents) | -1: a mix
static int perm_state(const FusedCall& c) {
    int with = 0;
    for (int i = 0; i < c.nmat; ++i) with += perm_of(c.wl[i]) ? 1 : 0;
    if (with == 0) return 0;
    if (with != c.nmat) return -1;
    for (int i = 1; i < c.nmat; ++i)
        if (!kperm_equal(&perm_of(c.wl[0])->h, &perm_of(c.wl[i])->h)) return -1;
    return 1;
}

// ---- the checks of the fused doors -----------------------------------------------------------------------------------------------
// Each rule is said once, with its message.  The ORDER in which a door asks them is the door's own -- fused_impl holds the outputs to
// their alignment before the activations, tmac_hip_qgemm_fused_xf_dev the other way round -- and a caller with two faults gets the
// message of the first: tests/golden/fused_refusals.json pins every door's order (tests/test_gpu_fused_refusals.py).
static int32_t args_check(const FusedCall& c) {
    if (!c.wl || !c.C || !c.B || c.nmat < 1 || c.nmat > 4 || c.N < 1) return fail(TMAC_HIP_E_ARG, "bad fused arguments (1..4 matrices)");
    return TMAC_HIP_OK;
}
int32_t tmac_host::nulls_check(const FusedCall& c) {
    for (int i = 0; i < c.nmat; ++i)
        if (!c.wl[i] || !c.C[i]) return fail(TMAC_HIP_E_ARG, "null matrix or output");
    return TMAC_HIP_OK;
}
// the alignment contract of the activations and the outputs (include/tmac_hip.h, "Alignment")
static int32_t act_align_check(const void* B_dev) {
    if (misaligned(B_dev, ACT_ALIGN)) return fail(TMAC_HIP_E_ARG, "B_dev must be %zu-byte aligned (the LUT build reads 16 bytes at a time)", ACT_ALIGN);
    return TMAC_HIP_OK;
}
static int32_t out_align_check(const FusedCall& c) {
    for (int i = 0; i < c.nmat; ++i)
        if (misaligned(c.C[i], out_align(c.out)))
            return fail(TMAC_HIP_E_ARG, "C_dev[%d] must be %zu-byte aligned (four outputs are stored at a time)", i, out_align(c.out));
    return TMAC_HIP_OK;
}
// one LUT, one kernel instantiation for all matrices of the call
static int32_t one_lut_check(const FusedCall& c) {
    for (int i = 0; i < c.nmat; ++i)
        if (!same_lut(c.wl[i], c.wl[0]) || !same_quant(c.wl[i], c.wl[0])) return fail(TMAC_HIP_E_ARG, "%s", ONE_LUT_MSG);
    return TMAC_HIP_OK;
}
// doors that do not serve act-order handles: refused by name
static int32_t refuse_perm(const FusedCall& c, const char* what) {
    for (int i = 0; c.wl && i < c.nmat; ++i)
        if (perm_of(c.wl[i])) return fail(TMAC_HIP_E_ARG, "matrix %d carries a K permutation (act-order): %s on such handles is not served yet", i, what);
    return TMAC_HIP_OK;
}
// (what k_gemv_quad's MFMA form takes, as the conditions a matrix misses: tmac_host.h)
unsigned tmac_host::quad_mfma_misses(const tmac_hip_weights* w) {
    return (g_knobs.variant == V_REF_LAYOUT ? QM_REF_VARIANT : 0u) | (g_knobs.variant == V_QUAD_MQSAD ? QM_MQSAD_VARIANT : 0u) |
           (layout_of(w->s) != L_QUAD || !w->tiled_ok ? QM_LAYOUT : 0u) | (w->fa ? QM_FAST_AGG : 0u) | (!gemv_quad_supported(w->s) ? QM_SHAPE : 0u);
}

// ---- handles with a bias (tmac_hip_weights_set_bias_dev) -----------------------------------------------------------------------
// y = W x + b is computed by k_gemv_quad's MFMA form (bias instantiations: LUT built in-kernel or copied) and by k_gemm_planes' per-group
// flavour, in front of the output's one store; every other kernel would drop the bias, so a plan that lands on one is refused, naming the
// route, before the first launch.  A call with a biased matrix is never recorded, never queued and never tapped (fused_impl); apart from
// that it takes the plan the plain call takes.
static int32_t bias_split_check(const tmac_hip_weights* w, Route r) {
    if (!w->bias) return TMAC_HIP_OK;
    if (r != R_GEMV_QUAD && r != R_GEMM_PLANES)
        return fail(TMAC_HIP_E_NOMATCH, "the matrix carries a bias, which %s does not add (k_gemv_quad's MFMA form and k_gemm_planes do)", ROUTE_NAMES[r]);
    if (r == R_GEMV_QUAD && quad_mfma_misses(w))
        return fail(TMAC_HIP_E_NOMATCH, "the matrix carries a bias, which k_gemv_quad adds in its MFMA form only (variant 0 or 6)");
    if (r == R_GEMV_QUAD) {      // the copy form's own plan, asked here so that a forced configuration it lacks is refused before any launch
        QuadPlan qp;
        if (!quad_plan_bias(w->s, w->s.nquads(), false, 0, g_knobs.force_ft, g_knobs.force_wpq, g_knobs.force_ft || g_knobs.force_wpq, qp))
            return fail(TMAC_HIP_E_NOMATCH, "the matrix carries a bias: no biased GEMV kernel copies the workspace's LUT in this configuration (copy form: (512,1), (512,2))");
    }
    return TMAC_HIP_OK;
}
static int32_t bias_plan_check(const Plan& p, const FusedCall& c) {
    if (!any_bias(c)) return TMAC_HIP_OK;
    if (p.route == R_ROW_LOOP) {
        // each matrix is planned again from the workspace's state (plan_split): the half-table build leaves no LUT image, the
        // three-layout build may -- asked both ways
        for (int i = 0; i < c.nmat; ++i)
            for (int img = 0; img <= (p.lut == LB_HALF_TABLES ? 0 : 1); ++img) {
                const Plan q = plan_split_on(c.wl[i], img != 0, c.N, false);
                if (q.err) return fail(q.err, q.msg, q.mat);
                const int32_t rc = bias_split_check(c.wl[i], q.route);
                if (rc) return rc;
            }
        return TMAC_HIP_OK;
    }
    if (p.route != R_GEMV_QUAD && p.route != R_GEMM_PLANES)
        return fail(TMAC_HIP_E_NOMATCH, "a matrix of the call carries a bias, which %s does not add (k_gemv_quad's MFMA form and k_gemm_planes do)", ROUTE_NAMES[p.route]);
    for (int i = 0; p.route == R_GEMV_QUAD && i < c.nmat; ++i)
        if (quad_mfma_misses(c.wl[i]) || c.wl[i]->s.m_groups >= 1)
            return fail(TMAC_HIP_E_NOMATCH, "a matrix of the call carries a bias, which k_gemv_quad adds in its MFMA form only (variant 0 or 6, per-group scales): matrix %d", i);
    return TMAC_HIP_OK;
}
// k_gemv_quad's bias block: the handles' own copies (null: the matrix has none)
template <class Args>
static void fill_bias(Args& fa, const FusedCall& c) {
    for (int i = 0; i < 4; ++i) fa.bias[i] = i < c.nmat ? c.wl[i]->bias : nullptr;
}
// A transform in front of a biased matrix: NORM and the silu GLU have instantiations with the add; the rule is the same for every N.
static int32_t xf_bias_check(const XfSpec& spec, const FusedCall& c) {
    if (!any_bias(c)) return TMAC_HIP_OK;
    if (spec.kind == TMAC_XF_GLU_NORM || spec.gate != 0)
        return fail(TMAC_HIP_E_NOMATCH, "a matrix of the call carries a bias: GLU_NORM and the relu^2 / GELU gates in front of a biased matrix are not served (NORM and the silu GLU are)");
    return TMAC_HIP_OK;
}

// ---- split entry point -----------------------------------------------------------------------------------------------------
int32_t tmac_host::qgemm_impl(const tmac_hip_weights* w, const tmac_hip_workspace* ws, void* C_dev, tmac_dtype_t out_dtype,
                          int N, int32_t* dump, hipStream_t st) {
    bind_thread_device();
    const int32_t brc = defer_barrier();       // behind the calling thread's deferred queue (the LUT may come from a queued output; C_dev may be one)
    if (brc) return brc;
    if (!w || !ws || !C_dev) return fail(TMAC_HIP_E_ARG, "null argument");
    if (misaligned(C_dev, out_align(out_dtype))) return fail(TMAC_HIP_E_ARG, "C_dev must be %zu-byte aligned (four outputs are stored at a time)", out_align(out_dtype));
    const LutHeld& held = ws->held;
    if (!held.serves_lut(w->s.K, w->s.ags, 1))
        return fail(TMAC_HIP_E_ARG, "workspace LUT (K=%d, ags=%d) does not match the weights (K=%d, ags=%d)", held.K(), held.ags(), w->s.K, w->s.ags);
    if (!held.serves_lut(w->s.K, w->s.ags, N)) return fail(TMAC_HIP_E_ARG, "N=%d but the workspace LUT holds %d rows", N, held.N());
    if (!held.built_through(perm_id_of(w)))
        return fail(TMAC_HIP_E_ARG, perm_of(w) ? "the weights carry a K permutation (act-order) but the workspace LUT was not built through it (tmac_hip_preprocessor_perm_dev)"
                                               : "the workspace LUT was built through a K permutation the weights do not carry");
    if (w->bias && dump) return fail(TMAC_HIP_E_ARG, "a parity tap on a handle that carries a bias is not served");
    const Plan p = plan_split(w, ws, N, dump != nullptr);
    if (p.err) return fail(p.err, p.msg, p.mat);
    const int32_t bias_rc = bias_split_check(w, p.route);
    if (bias_rc) return bias_rc;
    // the planned kernel reads tables somebody built: its layout of the LUT, or the LUT image, is in the workspace's record
    const bool planes = p.route == R_GEMM_PLANES;
    const LutLayout reads = p.route == R_REF_LAYOUT ? LUT_REF : p.route == R_GEMV_LO ? LUT_DEV : LUT_HALF;
    if (planes ? !held.serves_image(image_kind_for(w->s), w->s.K, N) : !held.has_layout(reads))
        return fail(TMAC_HIP_E_RUNTIME, "route %s reads %s, which the workspace's last LUT build did not write", ROUTE_NAMES[p.route],
                    planes ? "the LUT image" : reads == LUT_REF ? "qlut_ref" : reads == LUT_DEV ? "qlut_dev" : "the half-table image");
    count_route(p.route);
    void* cl[1] = {C_dev};
    const FusedCall one = one_matrix(&w, cl, out_dtype, N, st);
    switch (p.route) {
    case R_GEMM_PLANES: return planes_multi(one, ws, nullptr);
    case R_GEMM_ONEHOT: return gemm_multi(one, ws, dump);
    case R_GEMV_ROWS: return rows_multi(one, ws, nullptr);
    case R_GEMV_QUAD:
    case R_GEMV_FUSED: {
        FusedArgs fa;
        fill_fused_args(fa, one);
        fa.dump = dump;
        fa.qlut_lds = ws->qlut_lds; fa.lut_scales = ws->lut_scales; fa.lut_biases = ws->lut_biases;
        if (w->bias) {       // (R_GEMV_QUAD: bias_split_check) the copy form of the bias instantiations
            FusedBiasArgs fb;
            static_cast<FusedArgs&>(fb) = fa;
            fill_bias(fb, one);
            return fused_gemv_rc(launch_gemv_quad(fb, N, false, g_knobs.force_ft, g_knobs.force_wpq, g_knobs.force_ft || g_knobs.force_wpq, st),
                                 "no biased GEMV kernel for this configuration (copy form: (512,1), (512,2))", "biased gemv");
        }
        return fused_gemv_rc(p.route == R_GEMV_QUAD ? launch_gemv_quad(fa, N, false, g_knobs.force_ft, g_knobs.force_wpq, false, st)
                                                    : launch_gemv_fused(fa, N, false, st));
    }
    default: break;
    }
    GemvArgs a;
    a.s = w->s; a.N = N; a.qlut_dev = ws->qlut_dev; a.qlut_ref = ws->qlut_ref;
    a.lut_scales = ws->lut_scales; a.lut_biases = ws->lut_biases; a.C = C_dev; a.out_dtype = (Dtype)out_dtype;
    a.ps_dump = dump;
    a.fa_mode = w->fa;
    if (p.route == R_REF_LAYOUT) {
        a.W = w->A_ref; a.SC = w->S_ref; a.sc_dtype = w->ref_dtype;
    } else {
        a.W = w->W; a.SC = w->SC; a.sc_dtype = w->sc_dtype;
    }
    hipError_t e = launch_gemv(a, p.route == R_REF_LAYOUT ? V_REF_LAYOUT : g_knobs.variant == V_LO_SDWA ? V_LO_SDWA : V_LO_MQSAD, st);
    if (e == hipErrorInvalidValue) return fail(TMAC_HIP_E_NOMATCH, "no GEMV kernel for this configuration");
    if (e != hipSuccess) return fail(TMAC_HIP_E_RUNTIME, "gemv launch: %s", hipGetErrorString(e));
    return TMAC_HIP_OK;
}

extern "C" int32_t tmac_hip_qgemm_dev(const tmac_hip_weights* w, const tmac_hip_workspace* ws, void* C_dev,
                                      tmac_dtype_t out_dtype, int N, void* stream) {
    return qgemm_impl(w, ws, C_dev, out_dtype, N, nullptr, (hipStream_t)stream);
}

// ---- parity taps -----------------------------------------------------------------------------------------------------------
// One tap round trip: tap (cap elements; grown when too small, the pointer nulled first so that a failed allocation leaves nothing
// dangling) is filled with 0x7f bytes, launch(tap) runs, elems integers come back to host.  Once anything was enqueued the stream
// is synchronised -- or, after a failure, drained -- before the return: nothing of the call may still use the scratch that the
// caller frees next.
template <class Launch>
static int32_t run_tap(int32_t*& tap, size_t& cap, size_t elems, int32_t* host, hipStream_t st, const char* what, Launch launch) {
    if (cap < elems) {
        if (tap) (void)hipFree(tap);
        tap = nullptr; cap = 0;
        HIP_TRY(hipMalloc((void**)&tap, elems * sizeof(int32_t)));
        cap = elems;
    }
    hipError_t e = hipMemsetAsync(tap, 0x7f, elems * sizeof(int32_t), st);
    int32_t rc = e == hipSuccess ? launch(tap) : fail(TMAC_HIP_E_RUNTIME, "%s fill: %s", what, hipGetErrorString(e));
    if (rc == TMAC_HIP_OK) {
        e = hipMemcpyAsync(host, tap, elems * sizeof(int32_t), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) rc = fail(TMAC_HIP_E_RUNTIME, "%s readback: %s", what, hipGetErrorString(e));
    } else {
        (void)hipStreamSynchronize(st);
    }
    return rc;
}
// elements of the per-plane integer tap of the GEMV kernels and k_gemm_onehot
static size_t ps_elems(const Shape& s, int N) { return (size_t)N * s.M() * ((s.m_groups >= 1 && s.ags == s.K) ? 1 : (size_t)s.ngroups()); }

extern "C" int32_t tmac_hip_qgemm_partial_sums(const tmac_hip_weights* w, const tmac_hip_workspace* ws_c, int32_t* PS_host,
                                               int N, void* stream) {
    if (!w || !ws_c || !PS_host) return fail(TMAC_HIP_E_ARG, "null argument");
    auto* ws = const_cast<tmac_hip_workspace*>(ws_c);
    hipStream_t st = (hipStream_t)stream;
    DevBuf Ctmp;
    HIP_TRY(Ctmp.alloc(sizeof(float) * (size_t)N * w->s.Mw));
    return run_tap(ws->dump, ws->dump_elems, ps_elems(w->s, N), PS_host, st, "partial-sum",
                   [&](int32_t* tap) { return qgemm_impl(w, ws, Ctmp.p, TMAC_F32, N, tap, st); });
}

extern "C" int32_t tmac_hip_debug_gemm_stamps(unsigned long long* dev_buffer) {
    g_knobs.gemm_stamps = dev_buffer;
    return TMAC_HIP_OK;
}

extern "C" int32_t tmac_hip_debug_gemm_kernel(int which) {
    if (which < 0 || which > 3)
        return fail(TMAC_HIP_E_ARG, "gemm kernel selector must be 0 (auto), 1 (k_gemm_onehot), 2 / 3 (k_gemm_planes with eight- / four-wave workgroups)");
    g_knobs.gemm_kernel = which;
    return TMAC_HIP_OK;
}

// Parity tap of k_gemm_planes: the combined integer sums comb[n][o][kk] = sum_p 2^p PS_p it feeds into the fp32 chain.
extern "C" int32_t tmac_hip_debug_gemm_comb_sums(const tmac_hip_weights* w, const tmac_hip_workspace* ws_c, int32_t* comb_host,
                                                 int N, void* stream) {
    const int32_t brc = defer_barrier();
    if (brc) return brc;
    if (!w || !ws_c || !comb_host) return fail(TMAC_HIP_E_ARG, "null argument");
    auto* ws = const_cast<tmac_hip_workspace*>(ws_c);
    hipStream_t st = (hipStream_t)stream;
    if (!ws->held.serves_image(image_kind_for(w->s), w->s.K, N)) return fail(TMAC_HIP_E_ARG, "the workspace holds no LUT image for K=%d, N=%d", w->s.K, N);
    if (!planes_ok(w)) return fail(TMAC_HIP_E_NOMATCH, "k_gemm_planes does not cover this configuration");
    const size_t elems = (size_t)N * w->s.Mw * (w->s.m_groups >= 1 ? 1 : w->s.K / 64);
    DevBuf Ctmp;
    HIP_TRY(Ctmp.alloc(sizeof(float) * (size_t)N * w->s.Mw));
    void* cl[1] = {Ctmp.p};
    return run_tap(ws->dump, ws->dump_elems, elems, comb_host, st, "comb-sum",
                   [&](int32_t* tap) { return planes_multi(one_matrix(&w, cl, TMAC_F32, N, st), ws, tap); });
}

// ---- k_gemv_rows: knob, counter, the row-group rule, parity tap ------------------------------------------------------------
extern "C" int32_t tmac_hip_debug_rows_kernel(int mode) {
    if (mode < 0 || mode > 2) return fail(TMAC_HIP_E_ARG, "rows kernel mode must be 0 (auto), 1 (off) or 2 (forced)");
    g_knobs.rows_kernel = mode;
    return TMAC_HIP_OK;
}

extern "C" int32_t tmac_hip_debug_rows_stats(uint64_t* launches) {
    if (!launches) return fail(TMAC_HIP_E_ARG, "null argument");
    *launches = g_knobs.rows_launches;
    return TMAC_HIP_OK;
}

extern "C" int32_t tmac_hip_debug_rows_plan(int K, int m_groups, int N, int32_t* r_fit, int32_t* ngroups, int32_t* cap, int32_t* live,
                                            size_t* lds_bytes) {
    RowsPlan p;
    if (m_groups == 0 || m_groups < -1) return fail(TMAC_HIP_E_ARG, "m_groups must be -1 (per-group scales) or >= 1 (unified scales)");
    if (!rows_plan(K, N, p)) return fail(TMAC_HIP_E_ARG, "no row groups for K=%d, N=%d (K a multiple of 64 whose tables of two rows fit %zu bytes of LDS)", K, N, ROWS_LDS_MAX);
    if (r_fit) *r_fit = p.r_fit;
    if (ngroups) *ngroups = p.ngroups;
    if (lds_bytes) *lds_bytes = p.lds_bytes;
    for (int g = 0; g < p.ngroups; ++g) {
        const bool last = g == p.ngroups - 1;
        if (cap) cap[g] = last ? p.cap_last : p.r_fit;
        if (live) live[g] = last ? p.live_last : p.r_fit;
    }
    return TMAC_HIP_OK;
}

// Parity tap of k_gemv_rows: the integers as they enter the float part, in the row grouping of an untapped call of that N.
extern "C" int32_t tmac_hip_debug_rows_comb_sums(const tmac_hip_weights* w, const tmac_hip_workspace* ws_c, int32_t* comb_host,
                                                 int N, void* stream) {
    const int32_t brc = defer_barrier();
    if (brc) return brc;
    if (!w || !ws_c || !comb_host) return fail(TMAC_HIP_E_ARG, "null argument");
    auto* ws = const_cast<tmac_hip_workspace*>(ws_c);
    hipStream_t st = (hipStream_t)stream;
    if (!ws->held.serves_lut(w->s.K, w->s.ags, N)) return fail(TMAC_HIP_E_ARG, "the workspace holds no LUT for K=%d, N=%d", w->s.K, N);
    if (!rows_covers(w)) return fail(TMAC_HIP_E_NOMATCH, "k_gemv_rows does not cover this configuration");
    const size_t elems = (size_t)N * w->s.Mw * (w->s.m_groups >= 1 ? (size_t)w->s.bits : (size_t)w->s.K / 64);
    DevBuf Ctmp;
    HIP_TRY(Ctmp.alloc(sizeof(float) * (size_t)N * w->s.Mw));
    void* cl[1] = {Ctmp.p};
    return run_tap(ws->dump, ws->dump_elems, elems, comb_host, st, "rows comb-sum",
                   [&](int32_t* tap) { return rows_multi(one_matrix(&w, cl, TMAC_F32, N, st), ws, tap); });
}

// The LUT image of the workspace in plain layouts: half tables int8 [N][K/4][8], then lut_scales, lut_biases and the
// per-act-group entry sums, fp32 [N][K/64] each.
extern "C" int32_t tmac_hip_debug_gemm_image_read(const tmac_hip_workspace* ws, int8_t* half_tables_host, float* lut_scales_host,
                                                  float* lut_biases_host, float* entry_sums_host, int N, void* stream) {
    const int32_t brc = defer_barrier();
    if (brc) return brc;
    if (!ws || !half_tables_host || !lut_scales_host || !lut_biases_host || !entry_sums_host) return fail(TMAC_HIP_E_ARG, "null argument");
    const int K = ws->held.K(), Np = ws->gNpad;
    if (!ws->held.serves_image(ws->held.image(), K, N)) return fail(TMAC_HIP_E_ARG, "the workspace holds no LUT image for N=%d", N);
    hipStream_t st = (hipStream_t)stream;
    const bool rowwise = ws->held.image() == IMG_ROWWISE;           // one act group per row: k_preprocess_pairs_row's layout
    const int G = rowwise ? 1 : K / 64;
    std::vector<uint8_t> img((size_t)2 * K * Np);
    std::vector<float> col((size_t)(rowwise ? 3 : 4) * G * Np);
    HIP_TRY(hipMemcpyAsync(img.data(), ws->gimg, img.size(), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(col.data(), ws->gcol, col.size() * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int n = 0; n < N; ++n) {
        for (int t2 = 0; t2 < K / 8; ++t2) {           // pair t2 = tables 2 t2, 2 t2 + 1: unit t2 / 4, pair t2 % 4; act group t2 / 8, part t2 % 8
            const size_t u4 = rowwise ? ((size_t)(t2 >> 2) * 4 + (t2 & 3)) * Np + n
                                      : (((size_t)(t2 >> 3) * (Np >> 6) + (n >> 6)) * 8 + (t2 & 7)) * 64 + (n & 63);
            memcpy(half_tables_host + ((size_t)n * (K / 4) + 2 * t2) * 8, img.data() + u4 * 16, 16);
        }
        for (int kk = 0; kk < G; ++kk) {
            if (rowwise) {
                lut_scales_host[n] = col[n];
                lut_biases_host[n] = col[(size_t)Np + n];
                int32_t esi;                               // (int32 bits, see k_preprocess_pairs_row)
                memcpy(&esi, &col[(size_t)2 * Np + n], sizeof(esi));
                entry_sums_host[n] = (float)esi;
            } else {
                const float* c4 = &col[((size_t)kk * Np + n) * 4];        // lut_scales / 2 | lut_biases / 2 | entry sum | lut_biases
                lut_scales_host[(size_t)n * G + kk] = c4[0] * 2.0f;
                lut_biases_host[(size_t)n * G + kk] = c4[3];
                entry_sums_host[(size_t)n * G + kk] = c4[2];
            }
        }
    }
    return TMAC_HIP_OK;
}

// ---- fused entry point -----------------------------------------------------------------------------------------------------
// Prefill through the fused entry point: one LUT build into the stream's workspace, owned by the library (stream_workspace; tmac_hip_cache_clear()
// releases them), then the planned kernel.
// XfSpec -> the argument block of the row pass and of the XF LUT builders (the only place that knows XfRowsGateArgs' spelling of a
// transform: kind and gate side by side); r: the rows' 1 / rms, which k_xf_rows writes and the builders read
static void fill_xf_rows_args(XfRowsGateArgs& xa, const XfSpec& s, float* r) {
    memset(&xa, 0, sizeof(xa));
    xa.kind = s.kind; xa.gate = s.gate; xa.eps = s.eps;
    xa.in2 = s.in2; xa.residual = s.residual; xa.gamma = s.gamma; xa.residual_out = s.residual_out; xa.r = r;
}
// spec: the call carries a vector transform (N >= 2, plan_call's in_build): the row pass, then the planned LUT build's XF instantiation
// kp: the matrices carry this K permutation (N >= 2, plan_call's in_build, never with spec): the planned LUT build's gather instantiation
static int32_t fused_prefill(Plan p, const FusedCall& c, const XfSpec* spec = nullptr, const KPermData* kp = nullptr) {
    const Shape& s0 = c.s0();
    const int N = c.N;
    const hipStream_t st = c.st;
    tmac_hip_workspace* ws = nullptr;
    int32_t rc = stream_workspace(st, s0.K, N, &ws);
    if (rc) return rc;
    if (p.route == R_GEMM_PLANES && !ws->image_fits(s0.K)) {   // (see image_fits at the planners)
        p = plan_call(c, false, spec || kp, false);
        if (p.err) return fail(p.err, p.msg, p.mat);
        if ((rc = bias_plan_check(p, c)) != TMAC_HIP_OK) return rc;      // (the new plan's route must add the bias too; nothing is launched yet)
    }
    LutBuildReq q;
    q.K = s0.K; q.N = N; q.ags = s0.ags; q.want = p.lut; q.unified = s0.m_groups >= 1; q.xf = spec != nullptr;
    if (kp) { q.perm_id = kp->h.id; q.perm_K = kp->h.K; }      // (recorded: what the row loop's tmac_hip_qgemm_dev holds the matrices to)
    LutBuildPlan lb;
    rc = lut_build_plan(q, lut_caps(ws), &lb);
    if (rc) return rc;
    XfRowsGateArgs xa;
    if (spec) {
        fill_xf_rows_args(xa, *spec, ws->xf_r);
        if (xf_needs_row_pass(*spec)) {
            const hipError_t e = launch_xf_rows(xa, c.B, c.act_f16(), xa.gamma ? ws->xf_r : nullptr, s0.K, N, st);
            if (e != hipSuccess) return fail(TMAC_HIP_E_RUNTIME, "transform row pass launch: %s", hipGetErrorString(e));
        }
    }
    rc = lut_build(ws, lb, c.B, c.act, spec ? &xa : nullptr, kp ? kp->dev : nullptr, st);
    if (rc) return rc;
    count_route(p.route);
    if (p.route == R_GEMM_PLANES) return planes_multi(c, ws, nullptr);
    if (p.route == R_GEMM_ONEHOT) return gemm_multi(c, ws, nullptr);
    if (p.route == R_GEMV_ROWS) return rows_multi(c, ws, nullptr);
    for (int i = 0; i < c.nmat && rc == TMAC_HIP_OK; ++i) rc = tmac_hip_qgemm_dev(c.wl[i], ws, c.C[i], c.out, N, st);
    return rc;
}
// The one site that launches k_gemv_quad with an in-kernel LUT build, for the three argument blocks (FusedArgs, FusedXfArgs,
// FusedPermArgs): counts the route, fills what the call decides, lets the door add its own fields (extra), decides the launch
// configuration -- forced (tmac_hip_debug_quad_config), which is strict: the block must have that instantiation; else, for one row and no
// tap, the tuned one; else the heuristic -- launches, and words a failure the door's way.
template <class Args, class Extra>
static int32_t launch_quad(const FusedCall& c, Extra extra, const char* nomatch, const char* what) {
    count_route(R_GEMV_QUAD);
    Args fa;
    const int nb = fill_fused_args(fa, c);
    extra(fa);
    int ft = g_knobs.force_ft, wpq = g_knobs.force_wpq;
    const bool strict = ft || wpq;
    if (!strict && !fa.dump && c.N == 1) tuned_config(fa, nb, ft, wpq);
    return fused_gemv_rc(launch_gemv_quad(fa, c.N, true, ft, wpq, strict, c.st), nomatch, what);
}
// A fused call on matrices that all carry the same K permutation (fused_impl has checked that, the arguments and the alignment).  Behind
// the calling thread's deferred queue, stand-alone, like a call of several rows.  N = 1: k_gemv_quad's gather instantiations (the covered
// configurations and the fall-back of a transformed call).  N >= 2: routed as tmac_hip_qgemm_fused_xf_rows_dev routes a transformed call
// (plan_call's in_build), the planned LUT build gathering.
static int32_t fused_perm(const FusedCall& c) {
    const KPermData* kp = perm_of(c.wl[0]);
    for (int i = 0; i < c.nmat; ++i) {
        const tmac_hip_weights* w = c.wl[i];
        if (!c.C[i]) return fail(TMAC_HIP_E_ARG, "null matrix or output");
        if (quad_mfma_misses(w) || w->s.m_groups >= 1)
            return fail(TMAC_HIP_E_NOMATCH, "matrix %d: act-order handles run on k_gemv_quad's MFMA form and the prefill kernels behind it (QUAD layout, per-group scales)", i);
        if (!same_lut(w, c.wl[0]) || !same_quant(w, c.wl[0])) return fail(TMAC_HIP_E_ARG, "%s", ONE_LUT_MSG);
    }
    const Plan p = plan_call(c, false, true);
    if (p.err) return fail(p.err, p.msg, p.mat);
    if (c.N == 1 && p.route != R_GEMV_QUAD) return fail(TMAC_HIP_E_NOMATCH, "act-order handles of one row run on k_gemv_quad only");
    const int32_t brc = defer_barrier();
    if (brc) return brc;
    if (c.N >= 2) return fused_prefill(p, c, nullptr, kp);
    return launch_quad<FusedPermArgs>(c, [&](FusedPermArgs& fa) { fa.perm = kp->dev; },
                                      "no gathering GEMV kernel for this configuration (gather instantiations: (512,1), (512,2), (768,3), (1024,4))", "gathering gemv");
}
// A fused call with at least one biased matrix (fused_impl has checked the arguments and the alignment; no matrix carries a permutation:
// tmac_hip_weights_set_bias_dev refuses those).  The plan of the plain call, held to the routes that add a bias before anything is
// launched; behind the calling thread's deferred queue, stand-alone.
static int32_t fused_bias(const FusedCall& c) {
    const Plan p = plan_call(c, false);
    if (p.err) return fail(p.err, p.msg, p.mat);
    int32_t rc = bias_plan_check(p, c);
    if (rc) return rc;
    rc = defer_barrier();
    if (rc) return rc;
    if (p.route != R_GEMV_QUAD) return fused_prefill(p, c);
    return launch_quad<FusedBiasArgs>(c, [&](FusedBiasArgs& fa) { fill_bias(fa, c); },
                                      "no biased GEMV kernel for this configuration (bias instantiations: (512,1), (512,2), (768,3), (1024,4))", "biased gemv");
}
int32_t tmac_host::fused_impl(const FusedCall& c, int32_t* dump, float* lut_tap) {
    bind_thread_device();
    // the argument and alignment checks, ahead of the recorder, the deferred queue and the planner alike: a refused call is neither
    // recorded nor queued, launches nothing and leaves the queue as it is
    int32_t arc = args_check(c);
    if (arc == TMAC_HIP_OK) arc = out_align_check(c);
    if (arc == TMAC_HIP_OK) arc = act_align_check(c.B);
    if (arc) {
        if (chain_recording()) chain_clear_xform();      // a rejected call must not leave its transform pending for the next recorded call
        return arc;
    }
    const bool tap = dump || lut_tap;
    const int ps = perm_state(c);
    if (ps != 0) {        // act-order handles: never recorded, never queued, never tapped
        if (chain_recording()) chain_clear_xform();
        if (ps < 0) return fail(TMAC_HIP_E_ARG, "matrices fused in one launch must share the K permutation");
        if (tap) return refuse_perm(c, "a parity tap");
        if (chain_recording_independent()) {     // ... but noted where the recording can only become a stream: k_lut_images gathers (N = 1)
            for (int i = 0; i < c.nmat; ++i)
                if (c.wl[i]->s.m_groups >= 1) return fail(TMAC_HIP_E_NOMATCH, "matrix %d: act-order handles are served with per-group scales only", i);
            return chain_record(c);
        }
        if (chain_recording()) return refuse_perm(c, "a recorded call (tmac_hip_chain_begin ... _end)");
        return fused_perm(c);
    }
    if (any_bias(c)) {    // handles with a bias: never recorded (plain and declared-independent alike), never queued, never tapped
        if (chain_recording()) {
            chain_clear_xform();
            return fail(TMAC_HIP_E_ARG, "a matrix of the call carries a bias: such a call cannot be recorded (tmac_hip_chain_begin ... _end)");
        }
        if (tap) return fail(TMAC_HIP_E_ARG, "a matrix of the call carries a bias: a parity tap on such handles is not served");
        return fused_bias(c);
    }
    if (chain_recording() && !tap) return chain_record(c);
    if (!tap) {           // deferred launches: queued until tmac_hip_flush (or a call that depends on a queued one)
        int32_t drc;
        if (defer_if_on(c, &drc)) return drc;
    } else {              // a tap is never queued: it goes behind the queue (B_dev may be a queued output)
        const int32_t brc = defer_barrier();
        if (brc) return brc;
    }
    const Plan p = plan_call(c, tap);
    if (p.err) return fail(p.err, p.msg, p.mat);
    if (p.route != R_GEMV_QUAD && p.route != R_GEMV_FUSED) return fused_prefill(p, c);
    auto taps = [&](FusedArgs& fa) {
        fa.dump = dump;
        fa.stamps = g_knobs.stamps;
        if (g_knobs.stamps && !fa.dump) fa.dump = g_knobs.stamp_dump;   // the stamps live in the tap (DUMP) instantiation of the kernel
        fa.lut_tap = lut_tap;
    };
    if (p.route == R_GEMV_QUAD) return launch_quad<FusedArgs>(c, taps, "no fused GEMV kernel for this configuration", "fused gemv");
    count_route(p.route);
    FusedArgs fa;
    fill_fused_args(fa, c);
    taps(fa);
    return fused_gemv_rc(launch_gemv_fused(fa, c.N, true, c.st));
}
extern "C" int32_t tmac_hip_qgemm_fused_dev(const tmac_hip_weights* const* weights, int nmat, const void* B_dev,
                                            tmac_dtype_t act_dtype, void* const* C_dev, tmac_dtype_t out_dtype, int N,
                                            void* stream) {
    return fused_impl(FusedCall{weights, nmat, B_dev, act_dtype, C_dev, out_dtype, N, (hipStream_t)stream}, nullptr, nullptr);
}

// ---- fused entry point with a vector transform (N = 1) -----------------------------------------------------------------------
// Outside a recording: k_gemv_quad's XF instantiations.  Everything is checked before anything is launched; a transformed call is never
// queued (it goes behind the deferred queue like every non-hot entry point).
// The field rules are tmac_xform.h's (xf_resolve, xf_overlap_check); all of them come before anything about matrices, plans or routes.
// residual_out against what an N-row call on these matrices reads and writes
static int32_t xf_call_overlap_check(const XfSpec& spec, XfSite site, const FusedCall& c, const tmac_hip_xform* xf) {
    XfOut outs[4];
    for (int i = 0; i < c.nmat; ++i) outs[i] = XfOut{c.C[i], c.out_bytes(i)};
    return xf_overlap_check(spec, site, c.B, c.act_f16() ? 2 : 4, xf->in2, c.s0().K, c.N, outs, c.nmat);
}
// XfSpec -> the transform fields of k_gemv_quad's XF block (the only place that knows FusedXfArgs' spelling: the gate in bits 8.. of xf_kind)
static void fill_fused_xf_args(FusedXfArgs& fa, const XfSpec& s) {
    fa.xf_kind = s.kind | (s.gate << 8); fa.in2 = s.in2; fa.residual = s.residual; fa.gamma = s.gamma; fa.residual_out = s.residual_out; fa.eps = s.eps;
}
extern "C" int32_t tmac_hip_qgemm_fused_xf_dev(const tmac_hip_weights* const* wl, int nmat, const void* B_dev, tmac_dtype_t act_dtype,
                                               const tmac_hip_xform* xf, void* const* C_list, tmac_dtype_t out_dtype, void* stream) {
    const FusedCall c{wl, nmat, B_dev, act_dtype, C_list, out_dtype, 1, (hipStream_t)stream};
    const int32_t drc = ensure_device();
    if (drc) return drc;
    if (!xf || xf->kind == TMAC_XF_NONE) return fused_impl(c, nullptr, nullptr);
    if (chain_recording()) {       // one call site for both modes: the chain's own rules apply (CARRY allowed, fp16 in2)
        int32_t rc = tmac_hip_chain_xform(xf);
        if (rc == TMAC_HIP_OK) rc = fused_impl(c, nullptr, nullptr);
        if (rc != TMAC_HIP_OK && chain_recording()) chain_clear_xform();      // a rejected call leaves no pending transform
        return rc;
    }
    XfSpec spec;
    int32_t rc = xf_resolve(xf, XF_SITE_N1, &spec);
    if (rc || (rc = args_check(c)) != TMAC_HIP_OK || (rc = refuse_perm(c, "a vector transform")) != TMAC_HIP_OK) return rc;
    if ((rc = act_align_check(c.B)) != TMAC_HIP_OK || (rc = out_align_check(c)) != TMAC_HIP_OK || (rc = xf_bias_check(spec, c)) != TMAC_HIP_OK) return rc;
    const Plan p = plan_call(c, false, true);
    if (p.err) return fail(p.err, p.msg, p.mat);
    if (p.route != R_GEMV_QUAD || (quad_mfma_misses(wl[0]) & QM_MQSAD_VARIANT) || c.s0().K > QUAD_XF_MAX_K)
        return fail(TMAC_HIP_E_NOMATCH, "a transformed call runs on k_gemv_quad with the MFMA accumulate only (QUAD layout, K <= %d)", QUAD_XF_MAX_K);
    if ((rc = bias_plan_check(p, c)) != TMAC_HIP_OK) return rc;
    // (every workgroup reads the whole of the inputs while ONE workgroup writes each pair of residual_out: no order between the two)
    if ((rc = xf_call_overlap_check(spec, XF_SITE_N1, c, xf)) != TMAC_HIP_OK) return rc;
    bind_thread_device();
    const int32_t brc = defer_barrier();       // never queued: behind the calling thread's queue (B_dev may be a queued output)
    if (brc) return brc;
    if (any_bias(c))     // NORM or the silu GLU (xf_bias_check) in front of a biased matrix: the XF + BI instantiations
        return launch_quad<FusedXfBiasArgs>(c, [&](FusedXfBiasArgs& fa) { fill_fused_xf_args(fa, spec); fill_bias(fa, c); },
                                            "no transformed GEMV kernel with a bias for this configuration (instantiations: (512,1), (512,2), (768,3), (1024,4))",
                                            "transformed gemv with a bias");
    return launch_quad<FusedXfArgs>(c, [&](FusedXfArgs& fa) { fill_fused_xf_args(fa, spec); },
                                    "no transformed GEMV kernel for this configuration (XF instantiations: (512,1), (512,2), (768,3), (1024,4))", "transformed gemv");
}

// ---- fused entry point with a vector transform, N >= 1 rows ------------------------------------------------------------------
// N = 1 and "no transform" are the existing calls themselves.  N >= 2: every refusal comes before the first launch; then the row pass
// (k_xf_rows), the planned LUT build with the transform in its activation load, the planned kernel (fused_prefill).  Never recorded, never
// queued.
extern "C" int32_t tmac_hip_qgemm_fused_xf_rows_dev(const tmac_hip_weights* const* wl, int nmat, const void* B_dev, tmac_dtype_t act_dtype,
                                                    const tmac_hip_xform* xf, void* const* C_list, tmac_dtype_t out_dtype, int N, void* stream) {
    const FusedCall c{wl, nmat, B_dev, act_dtype, C_list, out_dtype, N, (hipStream_t)stream};
    const int32_t drc = ensure_device();
    if (drc) return drc;
    if (N == 1) return tmac_hip_qgemm_fused_xf_dev(wl, nmat, B_dev, act_dtype, xf, C_list, out_dtype, stream);
    if (!xf || xf->kind == TMAC_XF_NONE) return fused_impl(c, nullptr, nullptr);
    if (chain_recording()) {
        chain_clear_xform();           // (a transform declared for the next recorded call was meant for this one)
        return fail(TMAC_HIP_E_NOMATCH, "a transformed call of N=%d rows cannot be recorded: a chain takes one activation row", N);
    }
    int32_t rc = args_check(c);
    if (rc || (rc = nulls_check(c)) != TMAC_HIP_OK || (rc = refuse_perm(c, "a vector transform")) != TMAC_HIP_OK || (rc = out_align_check(c)) != TMAC_HIP_OK) return rc;
    const Shape& s0 = c.s0();
    XfSpec spec;
    if ((rc = xf_resolve(xf, XF_SITE_ROWS, &spec)) != TMAC_HIP_OK || (rc = act_align_check(c.B)) != TMAC_HIP_OK) return rc;
    if ((rc = xf_bias_check(spec, c)) != TMAC_HIP_OK) return rc;      // (the N = 1 door's rule: it does not depend on N)
    // (the builders read in, in2 and residual again after the row pass has written residual_out)
    if ((rc = xf_call_overlap_check(spec, XF_SITE_ROWS, c, xf)) != TMAC_HIP_OK || (rc = one_lut_check(c)) != TMAC_HIP_OK) return rc;
    // the scope: what the N = 1 form accepts (but for the accumulate, which the kernels behind the pair build choose), within the pair builds' reach
    if (quad_mfma_misses(wl[0]) & QM_REF_VARIANT) return fail(TMAC_HIP_E_NOMATCH, "a transformed call does not run on the reference layout");
    for (int i = 0; i < nmat; ++i) {
        const unsigned miss = quad_mfma_misses(wl[i]);
        if (miss & (QM_LAYOUT | QM_SHAPE))
            return fail(TMAC_HIP_E_NOMATCH, "matrix %d: a transformed call takes QUAD-layout weights of 1 to 4 bits with act groups of 64 or unified scales", i);
        if (miss & QM_FAST_AGG) return fail(TMAC_HIP_E_NOMATCH, "fast-aggregation weights do not take a transformed call");
    }
    if (s0.m_groups >= 1 && s0.K > PAIRS_ROW_MAX_K)
        return fail(TMAC_HIP_E_NOMATCH, "unified scales: K=%d is beyond the row-wise pair build (K <= %d)", s0.K, PAIRS_ROW_MAX_K);
    const Plan p = plan_call(c, false, true);
    if (p.err) return fail(p.err, p.msg, p.mat);
    if ((rc = bias_plan_check(p, c)) != TMAC_HIP_OK) return rc;       // (the transform lives in the LUT build, the bias in the kernel behind it)
    bind_thread_device();
    const int32_t brc = defer_barrier();       // never queued: behind the calling thread's queue (B_dev may be a queued output)
    if (brc) return brc;
    return fused_prefill(p, c, &spec);
}

// the two debug twins of plan_call: the plan's route and LUT form, or its refusal
static int32_t report_plan(const Plan& p, int32_t* route, int32_t* lut) {
    if (p.err) return fail(p.err, p.msg, p.mat);
    if (route) *route = (int32_t)p.route;
    if (lut) *lut = (int32_t)p.lut;
    return TMAC_HIP_OK;
}
// What a transformed call of N >= 2 rows on these matrices would run, by the rules of the call itself (host only: plans, launches nothing).
// route: 0 k_gemm_planes, 1 k_gemm_onehot, 3 k_gemv_rows, 7 the row loop (enum Route); lut: 1 the LUT image, 2 the half-table image.
extern "C" int32_t tmac_hip_debug_xf_rows_plan(const tmac_hip_weights* const* wl, int nmat, void* const* C_list, int N, int32_t* route, int32_t* lut) {
    if (!wl || !C_list || nmat < 1 || nmat > 4 || N < 2) return fail(TMAC_HIP_E_ARG, "bad plan arguments (1..4 matrices, N >= 2)");
    return report_plan(plan_call(FusedCall{wl, nmat, nullptr, TMAC_F32, C_list, TMAC_F32, N, nullptr}, false, true), route, lut);
}

// What an untransformed fused call on these matrices would run: plan_fused's answer as the call gets it (host only: plans, launches nothing).
// route: enum Route; lut: enum LutBuild.
extern "C" int32_t tmac_hip_debug_fused_plan(const tmac_hip_weights* const* wl, int nmat, void* const* C_list, int N, int32_t* route, int32_t* lut) {
    if (!wl || !C_list || nmat < 1 || nmat > 4 || N < 1) return fail(TMAC_HIP_E_ARG, "bad plan arguments (1..4 matrices, N >= 1)");
    return report_plan(plan_call(FusedCall{wl, nmat, nullptr, TMAC_F32, C_list, TMAC_F32, N, nullptr}, false), route, lut);
}

extern "C" int32_t tmac_hip_debug_route_stats(uint64_t counts[8]) {
    if (!counts) return fail(TMAC_HIP_E_ARG, "null argument");
    static_assert(R_ROW_LOOP == 7, "tmac_hip_debug_route_stats documents eight routes (include/tmac_hip.h)");
    for (int r = 0; r <= R_ROW_LOOP; ++r) counts[r] = g_knobs.route_launches[r];
    return TMAC_HIP_OK;
}

// The fp32 x [N][K] that the LUT builders of a transformed call consume: the row pass plus a store around the builders' own load
// (xf_rows_x8).  residual_out is written as the call would write it.
extern "C" int32_t tmac_hip_debug_xf_rows(const void* B_dev, tmac_dtype_t act_dtype, const tmac_hip_xform* xf, int K, int N, float* x_out_dev,
                                          void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const int32_t drc = ensure_device();
    if (drc) return drc;
    bind_thread_device();
    const int32_t brc = defer_barrier();
    if (brc) return brc;
    if (!B_dev || !xf || !x_out_dev || K <= 0 || K % 64 || N < 1) return fail(TMAC_HIP_E_ARG, "bad tap arguments (K a multiple of 64, N >= 1)");
    if (xf->kind == TMAC_XF_NONE) return fail(TMAC_HIP_E_ARG, "the tap shows a transform: kind NORM, GLU or GLU_NORM");
    XfSpec spec;
    int32_t rc = xf_resolve(xf, XF_SITE_ROWS, &spec);
    if (rc || (rc = act_align_check(B_dev)) != TMAC_HIP_OK) return rc;
    if (misaligned(x_out_dev, XFORM_ALIGN)) return fail(TMAC_HIP_E_ARG, "x_out_dev must be %zu-byte aligned", XFORM_ALIGN);
    const int f16 = act_dtype == TMAC_F16;
    const XfOut x_out{x_out_dev, (size_t)N * K * 4};
    if ((rc = xf_overlap_check(spec, XF_SITE_ROWS, B_dev, f16 ? 2 : 4, xf->in2, K, N, &x_out, 1, "x_out_dev")) != TMAC_HIP_OK) return rc;
    DevBuf r;
    if (spec.gamma) HIP_TRY(r.alloc(sizeof(float) * (size_t)N));
    XfRowsGateArgs xa;
    fill_xf_rows_args(xa, spec, r.as<float>());
    hipError_t e = hipSuccess;
    if (xf_needs_row_pass(spec)) e = launch_xf_rows(xa, B_dev, f16, r.as<float>(), K, N, st);
    if (e == hipSuccess) e = launch_xf_rows_tap(xa, B_dev, f16, x_out_dev, K, N, st);
    const hipError_t es = hipStreamSynchronize(st);      // r is freed on return
    if (e != hipSuccess || es != hipSuccess) return fail(TMAC_HIP_E_RUNTIME, "transform tap: %s", hipGetErrorString(e != hipSuccess ? e : es));
    return TMAC_HIP_OK;
}

extern "C" int32_t tmac_hip_qgemm_fused_partial_sums(const tmac_hip_weights* w, const void* B_dev, tmac_dtype_t act_dtype,
                                                     int32_t* PS_host, float* C_host, float* lut_host, int N, void* stream) {
    if (!w || !PS_host) return fail(TMAC_HIP_E_ARG, "null argument");
    hipStream_t st = (hipStream_t)stream;
    DevBuf Ctmp, ltap;
    const size_t lt = (size_t)N * 2 * w->s.ngroups();
    HIP_TRY(ltap.alloc(lt * sizeof(float)));
    HIP_TRY(Ctmp.alloc(sizeof(float) * (size_t)N * w->s.Mw));
    void* cl[1] = {Ctmp.p};
    int32_t* tap = nullptr;      // scratch of this call, unlike the workspace's tap of the two entry points above
    size_t cap = 0;
    int32_t rc = run_tap(tap, cap, ps_elems(w->s, N), PS_host, st, "fused tap",
                         [&](int32_t* t) { return fused_impl(FusedCall{&w, 1, B_dev, act_dtype, cl, TMAC_F32, N, st}, t, ltap.as<float>()); });
    if (tap) (void)hipFree(tap);
    if (rc) return rc;
    if (C_host) HIP_TRY(hipMemcpy(C_host, Ctmp.p, sizeof(float) * (size_t)N * w->s.Mw, hipMemcpyDeviceToHost));
    if (lut_host) HIP_TRY(hipMemcpy(lut_host, ltap.p, lt * sizeof(float), hipMemcpyDeviceToHost));
    return TMAC_HIP_OK;
}
