// tmac_experts.cpp — expert banks (tmac_hip_bank_*) and the entry points of a mixture-of-experts layer's top-k GEMVs:
// tmac_hip_qgemm_experts_dev -- check the call, build the half-table image of its activation rows into the stream's library workspace
// with the existing builder, then ONE k_gemv_experts launch (tmac_experts.hip) that picks every slot's matrix on the device -- and
// tmac_hip_qgemm_experts_fused_dev -- the same checks, then that launch alone: the kernel builds its tables itself, optionally behind a
// GLU.  Nothing here reads ids or gates.  DESIGN.md 4.17.
#include "tmac_host.h"
#include "tmac_select.h"

using namespace tmac_host;

// E interchangeable matrices of one projection.  `experts`: the handles as given (the caller keeps them registered while the bank lives:
// a handle has no reference count of its own; ExpertBank of the Python layer holds its Weights objects); `tab`: the device table.
struct tmac_hip_bank {
    std::vector<const tmac_hip_weights*> experts;
    ExpertEntry* tab = nullptr;
    Shape s;                       // of expert 0: every expert has the same
    Dtype sc_dtype = F32;
};

// what of expert i differs from expert 0 (null: nothing a launch depends on)
static const char* bank_mismatch(const tmac_hip_weights* w, const tmac_hip_weights* w0) {
    const Shape &a = w->s, &b = w0->s;
    if (a.Mw != b.Mw) return "Mw";
    if (a.K != b.K) return "K";
    if (a.bits != b.bits) return "bits";
    if (a.gs != b.gs || a.ags != b.ags) return "group size";
    if (a.zero_point != b.zero_point) return "zero-point setting";
    if (w->sc_dtype != w0->sc_dtype) return "scale dtype";
    return nullptr;
}

extern "C" int32_t tmac_hip_bank_create(tmac_hip_bank** out, const tmac_hip_weights* const* experts, int E, void* stream) {
    if (!out || !experts) return fail(TMAC_HIP_E_ARG, "null argument");
    if (E < 1) return fail(TMAC_HIP_E_ARG, "a bank holds at least one expert (E=%d)", E);
    int32_t rc = ensure_device();
    if (rc) return rc;
    for (int i = 0; i < E; ++i) {
        const tmac_hip_weights* w = experts[i];
        if (!w) return fail(TMAC_HIP_E_ARG, "expert %d: null handle", i);
        if (w->s.m_groups >= 1) return fail(TMAC_HIP_E_NOMATCH, "expert %d: unified-scale (BitNet) handles are not served in a bank", i);
        if (quad_mfma_misses(w) & (QM_LAYOUT | QM_FAST_AGG | QM_SHAPE))
            return fail(TMAC_HIP_E_NOMATCH, "expert %d: outside what k_gemv_quad's layout serves (QUAD layout, K a multiple of 64 up to 24576, Mw of 4, group sizes 64 x 2^n, exact sums)", i);
        if (w->bias) return fail(TMAC_HIP_E_ARG, "expert %d: handles with a bias are not served in a bank", i);
        if (w->kperm) return fail(TMAC_HIP_E_ARG, "expert %d: act-order handles (a K permutation) are not served in a bank", i);
        if (const char* what = bank_mismatch(w, experts[0])) return fail(TMAC_HIP_E_ARG, "expert %d: %s differs from expert 0's", i, what);
    }
    const hipStream_t st = (hipStream_t)stream;
    std::vector<ExpertEntry> host((size_t)E);
    for (int i = 0; i < E; ++i) host[i] = ExpertEntry{(const uint4*)experts[i]->W, experts[i]->SC};
    auto bank = std::make_unique<tmac_hip_bank>();
    bank->experts.assign(experts, experts + E);
    bank->s = experts[0]->s; bank->sc_dtype = experts[0]->sc_dtype;
    HIP_TRY(hipMalloc((void**)&bank->tab, sizeof(ExpertEntry) * (size_t)E));
    hipError_t e = hipMemcpyAsync(bank->tab, host.data(), sizeof(ExpertEntry) * (size_t)E, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);      // `host` leaves scope; the table is complete before its first reader on any stream
    if (e != hipSuccess) {
        (void)hipFree(bank->tab);
        return fail(TMAC_HIP_E_RUNTIME, "bank table upload: %s", hipGetErrorString(e));
    }
    *out = bank.release();
    return TMAC_HIP_OK;
}

extern "C" int32_t tmac_hip_bank_free(tmac_hip_bank* bank) {
    if (!bank) return TMAC_HIP_OK;
    if (bank->tab) (void)hipFree(bank->tab);
    delete bank;
    return TMAC_HIP_OK;
}

extern "C" int32_t tmac_hip_bank_info(const tmac_hip_bank* bank, int* E, int* Mw, int* K, int* bits) {
    if (!bank) return fail(TMAC_HIP_E_ARG, "null bank");
    if (E) *E = (int)bank->experts.size();
    if (Mw) *Mw = bank->s.Mw;
    if (K) *K = bank->s.K;
    if (bits) *bits = bank->s.bits;
    return TMAC_HIP_OK;
}

extern "C" int32_t tmac_hip_debug_experts_plan(int K, int bits, int group_size, const int* bank_Mw, int nbanks, int S, int lut_rows, int combine,
                                               int32_t* wpq, int32_t* grid, int32_t* items, size_t* lds_bytes) {
    if (!bank_Mw) return fail(TMAC_HIP_E_ARG, "null argument");
    Shape s{};
    s.K = K; s.bits = bits; s.gs = group_size; s.ags = 64; s.m_groups = -1; s.zero_point = 1;
    set_layout(s, L_QUAD);
    ExpertsPlan p;
    if (!experts_plan(s, bank_Mw, nbanks, S, lut_rows, combine ? EXPERTS_COMBINE : EXPERTS_SLOTS, p)) return fail(TMAC_HIP_E_NOMATCH, "experts call: %s", p.why);
    if (wpq) *wpq = p.wpq;
    if (grid) *grid = p.gx;
    if (items) *items = p.items;
    if (lds_bytes) *lds_bytes = p.lds_bytes;
    return TMAC_HIP_OK;
}

// ---- token batches: routing and gated sum.  Nothing here reads ids, the routing or gates. ------------------------------
extern "C" int32_t tmac_hip_experts_rows_sizes(int N, int S, int E, int32_t* T_max, int32_t* P) {
    ExpertsRowsSizes z;
    if (!experts_rows_sizes(N, S, E, z)) return fail(TMAC_HIP_E_ARG, "experts routing (N=%d, S=%d, E=%d): %s", N, S, E, z.why);
    if (T_max) *T_max = z.T_max;
    if (P) *P = z.P;
    return TMAC_HIP_OK;
}

extern "C" int32_t tmac_hip_experts_route_dev(const int32_t* ids_dev, int N, int S, int E, int32_t* tile_expert_dev, int32_t* src_dev, int32_t* pos_dev,
                                              void* stream) {
    bind_thread_device();
    if (!ids_dev || !tile_expert_dev || !src_dev || !pos_dev) return fail(TMAC_HIP_E_ARG, "null ids or routing output");
    ExpertsRowsSizes z;
    if (!experts_rows_sizes(N, S, E, z)) return fail(TMAC_HIP_E_ARG, "experts routing (N=%d, S=%d, E=%d): %s", N, S, E, z.why);
    if (chain_recording()) return fail(TMAC_HIP_E_ARG, "tmac_hip_experts_route_dev cannot be recorded (tmac_hip_chain_begin ... _end): expert calls run stand-alone");
    if (misaligned(ids_dev, 4) || misaligned(tile_expert_dev, 4) || misaligned(src_dev, 4) || misaligned(pos_dev, 4))
        return fail(TMAC_HIP_E_ARG, "ids_dev and the routing outputs must be 4-byte aligned");
    const int32_t rc = defer_barrier();
    if (rc) return rc;
    const hipError_t e = launch_experts_route(ids_dev, N * S, E, z.T_max, tile_expert_dev, src_dev, pos_dev, (hipStream_t)stream);
    if (e != hipSuccess) return fail(TMAC_HIP_E_RUNTIME, "experts routing launch: %s", hipGetErrorString(e));
    return TMAC_HIP_OK;
}

extern "C" int32_t tmac_hip_experts_combine_dev(const float* C_dev, const int32_t* pos_dev, const float* gates_dev, int N, int S, int Mw, int P, void* y_dev,
                                                tmac_dtype_t out_dtype, void* stream) {
    bind_thread_device();
    if (!C_dev || !pos_dev || !gates_dev || !y_dev) return fail(TMAC_HIP_E_ARG, "null argument");
    ExpertsRowsSizes z;
    if (!experts_rows_sizes(N, S, 1, z)) return fail(TMAC_HIP_E_ARG, "experts combine (N=%d, S=%d): %s", N, S, z.why);
    if (Mw < 4 || Mw % 4 != 0 || P < 64 || P % 64 != 0) return fail(TMAC_HIP_E_ARG, "experts combine: Mw=%d must be a multiple of 4, P=%d of 64", Mw, P);
    if (chain_recording()) return fail(TMAC_HIP_E_ARG, "tmac_hip_experts_combine_dev cannot be recorded (tmac_hip_chain_begin ... _end): expert calls run stand-alone");
    if (misaligned(C_dev, 16) || misaligned(y_dev, out_align(out_dtype)))
        return fail(TMAC_HIP_E_ARG, "C_dev must be 16-byte and y_dev %zu-byte aligned (four values are loaded and stored at a time)", out_align(out_dtype));
    if (misaligned(pos_dev, 4) || misaligned(gates_dev, 4)) return fail(TMAC_HIP_E_ARG, "pos_dev and gates_dev must be 4-byte aligned");
    const int32_t rc = defer_barrier();
    if (rc) return rc;
    const hipError_t e = launch_experts_combine(C_dev, pos_dev, gates_dev, N, S, Mw, P, y_dev, out_dtype == TMAC_F16, (hipStream_t)stream);
    if (e != hipSuccess) return fail(TMAC_HIP_E_RUNTIME, "experts combine launch: %s", hipGetErrorString(e));
    return TMAC_HIP_OK;
}

// ---- the fused router in front of both: logits, softmax and top-S in one launch (k_experts_router).  Nothing of the
//      library workspace is created, read or invalidated; nothing is read on the host. -------------------------------------------------------
// dtypes and the plan of a router call, or the refusal that names the field (pure)
static int32_t router_plan_check(int K, int E, int S, int N, tmac_dtype_t w_dtype, tmac_dtype_t act_dtype, ExpertsRouterPlan& p) {
    if ((w_dtype != TMAC_F16 && w_dtype != TMAC_F32) || (act_dtype != TMAC_F16 && act_dtype != TMAC_F32))
        return fail(TMAC_HIP_E_ARG, "experts router: w_dtype and act_dtype must be TMAC_F32 or TMAC_F16");
    if (!experts_router_plan(K, E, S, N, act_dtype == TMAC_F16, w_dtype == TMAC_F16, p))
        return fail(TMAC_HIP_E_ARG, "experts router (N=%d, K=%d, E=%d, S=%d): %s", N, K, E, S, p.why);
    return TMAC_HIP_OK;
}

extern "C" int32_t tmac_hip_debug_experts_router_plan(int K, int E, int S, int N, tmac_dtype_t w_dtype, tmac_dtype_t act_dtype, int32_t* waves,
                                                      int32_t* col_tiles, int32_t* k_slices, int32_t* steps_per_slice, int32_t* grid, size_t* lds_bytes) {
    ExpertsRouterPlan p;
    const int32_t rc = router_plan_check(K, E, S, N, w_dtype, act_dtype, p);
    if (rc) return rc;
    if (waves) *waves = p.waves;
    if (col_tiles) *col_tiles = p.ctiles;
    if (k_slices) *k_slices = p.slices;
    if (steps_per_slice) *steps_per_slice = p.steps;
    if (grid) *grid = p.gx;
    if (lds_bytes) *lds_bytes = p.lds_bytes;
    return TMAC_HIP_OK;
}

extern "C" int32_t tmac_hip_experts_router_dev(const void* Wr_dev, tmac_dtype_t w_dtype, const void* x_dev, tmac_dtype_t act_dtype, int N, int K, int E, int S,
                                               uint32_t flags, int32_t* ids_dev, float* gates_dev, float* logits_dev, void* stream) {
    const int32_t drc = ensure_device();
    if (drc) return drc;
    if (!Wr_dev || !x_dev || !ids_dev || !gates_dev) return fail(TMAC_HIP_E_ARG, "null Wr_dev, x_dev, ids_dev or gates_dev");
    if (flags & ~(uint32_t)TMAC_ROUTER_RENORM) return fail(TMAC_HIP_E_ARG, "flags=0x%x: unknown bits (TMAC_ROUTER_RENORM is the one flag)", flags);
    ExpertsRouterPlan p;
    const int32_t prc = router_plan_check(K, E, S, N, w_dtype, act_dtype, p);
    if (prc) return prc;
    if (misaligned(Wr_dev, ACT_ALIGN) || misaligned(x_dev, ACT_ALIGN))
        return fail(TMAC_HIP_E_ARG, "Wr_dev and x_dev must be %zu-byte aligned (rows are read 16 bytes at a time)", ACT_ALIGN);
    if (misaligned(ids_dev, 4) || misaligned(gates_dev, 4) || misaligned(logits_dev, 4))
        return fail(TMAC_HIP_E_ARG, "ids_dev, gates_dev and logits_dev must be 4-byte aligned");
    if (chain_recording()) return fail(TMAC_HIP_E_ARG, "tmac_hip_experts_router_dev cannot be recorded (tmac_hip_chain_begin ... _end): expert calls run stand-alone");
    const int32_t rc = defer_barrier();       // never queued: behind the calling thread's queue (x_dev may be a queued call's output)
    if (rc) return rc;
    ExpertsRouterArgs a;
    a.Wr = Wr_dev; a.x = x_dev; a.w_f16 = w_dtype == TMAC_F16; a.x_f16 = act_dtype == TMAC_F16;
    a.N = N; a.K = K; a.E = E; a.S = S; a.renorm = (flags & TMAC_ROUTER_RENORM) != 0;
    a.ids = ids_dev; a.gates = gates_dev; a.logits = logits_dev;
    const hipError_t e = launch_experts_router(a, p, (hipStream_t)stream);
    if (e != hipSuccess) return fail(TMAC_HIP_E_RUNTIME, "experts router launch: %s", hipGetErrorString(e));
    return TMAC_HIP_OK;
}

hipError_t tmac::launch_gemv_experts(const ExpertsArgs& a_in, hipStream_t st) {
    ExpertsArgs a = a_in;
    const Shape& s = a.s;
    const int mode = a.gates ? EXPERTS_COMBINE : EXPERTS_SLOTS;
    int Mw[EXPERTS_MAX_BANKS] = {0, 0};
    if (a.nbanks < 1 || a.nbanks > EXPERTS_MAX_BANKS) return hipErrorInvalidValue;
    for (int b = 0; b < a.nbanks; ++b) Mw[b] = a.b[b].Mw;
    ExpertsPlan p;
    if (!experts_plan(s, Mw, a.nbanks, a.S, a.lut_rows, mode, p)) return hipErrorInvalidValue;
    a.nu = s.K / 32; a.nst = (a.nu + 63) / 64; a.tstride = ((a.nu + 15) & ~15) + 1;
    a.G = s.K / s.ags; a.nsg = s.K / s.gs;
    a.gs_shift = 0;
    for (int g = s.gs / 32; g > 1; g >>= 1) ++a.gs_shift;
    int q = 0;
    for (int b = 0; b < a.nbanks; ++b) {
        // fragment offsets are 32-bit buffer offsets
        if ((size_t)(Mw[b] / 4) * a.nst * s.bits * 1024 >= ((size_t)1 << 31)) return hipErrorInvalidValue;
        q += Mw[b] / 4;
        a.b[b].q_end = q;
    }
    a.wpq = p.wpq;
    return sel_int<1, 2, 3, 4>(s.bits, [&](auto BITS) { return launch_gemv_experts_unit<decltype(BITS)::value>(a, p, mode, st); });
}

// The checks the two top-k entry points share, in the order tmac_hip_qgemm_experts_dev always made them (`fn` names the entry point in the
// messages), then the argument block without its table source and the plan.  Launches nothing, flushes nothing.
static int32_t experts_call_check(const char* fn, const tmac_hip_bank* const* banks, int nbanks, const void* B_dev, int lut_rows, const int32_t* ids_dev,
                                  const float* gates_dev, int S, void* const* C_dev, tmac_dtype_t out_dtype, ExpertsArgs& a) {
    if (!banks || !C_dev || nbanks < 1 || nbanks > EXPERTS_MAX_BANKS) return fail(TMAC_HIP_E_ARG, "%s takes one or two banks (nbanks=%d)", fn, nbanks);
    for (int b = 0; b < nbanks; ++b)
        if (!banks[b] || !C_dev[b]) return fail(TMAC_HIP_E_ARG, "null bank or output");
    if (!B_dev || !ids_dev) return fail(TMAC_HIP_E_ARG, "null activations or ids");
    if (chain_recording()) return fail(TMAC_HIP_E_ARG, "%s cannot be recorded (tmac_hip_chain_begin ... _end): expert calls run stand-alone", fn);
    if (S < 1 || S > EXPERTS_MAX_SLOTS) return fail(TMAC_HIP_E_ARG, "S=%d: an experts call takes 1 to %d slots", S, EXPERTS_MAX_SLOTS);
    if (lut_rows != 1 && lut_rows != S) return fail(TMAC_HIP_E_ARG, "lut_rows=%d: 1 (one activation row shared by the slots) or S=%d", lut_rows, S);
    const bool combine = gates_dev != nullptr;
    if (combine && nbanks != 1) return fail(TMAC_HIP_E_ARG, "COMBINE (gates given) takes one bank, the call has %d", nbanks);
    if (combine && lut_rows != S) return fail(TMAC_HIP_E_ARG, "COMBINE (gates given) takes one activation row per slot: lut_rows=%d, S=%d", lut_rows, S);
    for (int b = 0; b < nbanks; ++b)
        if (misaligned(C_dev[b], out_align(out_dtype)))
            return fail(TMAC_HIP_E_ARG, "C_dev[%d] must be %zu-byte aligned (four outputs are stored at a time)", b, out_align(out_dtype));
    if (misaligned(B_dev, ACT_ALIGN)) return fail(TMAC_HIP_E_ARG, "B_dev must be %zu-byte aligned (the LUT build reads 16 bytes at a time)", ACT_ALIGN);
    if (misaligned(ids_dev, 4) || misaligned(gates_dev, 4)) return fail(TMAC_HIP_E_ARG, "ids_dev and gates_dev must be 4-byte aligned");
    const tmac_hip_bank* b0 = banks[0];
    const Shape& s0 = b0->s;
    if (nbanks == 2) {
        const Shape& s1 = banks[1]->s;
        if (s1.K != s0.K || s1.bits != s0.bits || s1.gs != s0.gs || s1.ags != s0.ags || s1.zero_point != s0.zero_point || banks[1]->sc_dtype != b0->sc_dtype)
            return fail(TMAC_HIP_E_ARG, "banks of one call share K, bits, group size, zero-point setting and scale dtype (their rows may differ)");
    }
    memset(&a, 0, sizeof(a));
    int Mw[EXPERTS_MAX_BANKS] = {0, 0};
    for (int b = 0; b < nbanks; ++b) {
        Mw[b] = banks[b]->s.Mw;
        a.b[b].tab = banks[b]->tab; a.b[b].C = C_dev[b]; a.b[b].E = (int)banks[b]->experts.size(); a.b[b].Mw = Mw[b];
    }
    ExpertsPlan p;
    if (!experts_plan(s0, Mw, nbanks, S, lut_rows, combine ? EXPERTS_COMBINE : EXPERTS_SLOTS, p))
        return fail(TMAC_HIP_E_NOMATCH, "experts call (K=%d, S=%d, lut_rows=%d): %s", s0.K, S, lut_rows, p.why);
    a.nbanks = nbanks; a.s = s0;
    a.ids = ids_dev; a.gates = gates_dev; a.S = S; a.lut_rows = lut_rows;
    a.sc_f16 = b0->sc_dtype == F16; a.out_f16 = out_dtype == TMAC_F16;
    return TMAC_HIP_OK;
}

static int32_t experts_launch(const ExpertsArgs& a, hipStream_t st) {
    const hipError_t e = launch_gemv_experts(a, st);
    if (e == hipErrorInvalidValue) return fail(TMAC_HIP_E_NOMATCH, "experts kernel: configuration or sizes not covered (an expert's matrix must stay below 2 GB)");
    if (e != hipSuccess) return fail(TMAC_HIP_E_RUNTIME, "experts kernel launch: %s", hipGetErrorString(e));
    return TMAC_HIP_OK;
}

extern "C" int32_t tmac_hip_qgemm_experts_dev(const tmac_hip_bank* const* banks, int nbanks, const void* B_dev, tmac_dtype_t act_dtype, int lut_rows,
                                              const int32_t* ids_dev, const float* gates_dev, int S, void* const* C_dev, tmac_dtype_t out_dtype,
                                              void* stream) {
    bind_thread_device();
    // every check before anything is launched or flushed: a refused call launches nothing and leaves the deferred queue as it is
    ExpertsArgs a;
    int32_t rc = experts_call_check("tmac_hip_qgemm_experts_dev", banks, nbanks, B_dev, lut_rows, ids_dev, gates_dev, S, C_dev, out_dtype, a);
    if (rc) return rc;
    rc = defer_barrier();                     // never queued: behind the calling thread's queue (B_dev, ids_dev may be a queued call's output)
    if (rc) return rc;
    // the half-table image of the call's rows, by the builder k_gemv_rows is fed by
    const hipStream_t st = (hipStream_t)stream;
    const Shape& s0 = a.s;
    tmac_hip_workspace* ws = nullptr;
    if ((rc = stream_workspace(st, s0.K, lut_rows, &ws)) != TMAC_HIP_OK) return rc;
    LutBuildReq q;
    q.K = s0.K; q.N = lut_rows; q.ags = s0.ags; q.want = LB_HALF_TABLES;
    LutBuildPlan lb;
    if ((rc = lut_build_plan(q, lut_caps(ws), &lb)) != TMAC_HIP_OK) return rc;
    if ((rc = lut_build(ws, lb, B_dev, act_dtype, nullptr, nullptr, st)) != TMAC_HIP_OK) return rc;
    a.qlut_lds = ws->qlut_lds; a.lut_scales = ws->lut_scales; a.lut_biases = ws->lut_biases;
    return experts_launch(a, st);
}

// ---- the same call with its tables built in the launch (k_gemv_experts LUTSRC 1), optionally behind x = gate(in) * in2 (LUTSRC 2): one
//      launch, no workspace -- nothing of the stream's workspace is read, written or created, so the call may be the first thing a
//      capturing stream sees.  The plan is experts_plan's: it does not know how the tables are made.
// The transform of such a call: NONE or a GLU.  NORM and GLU_NORM are refused by name before their own field rules are looked at; kind,
// gate, the GLU's in2 and its alignment are the resolver's; a GLU reads one row of in and in2 per slot.
static int32_t experts_xf_check(const tmac_hip_xform* xf, int lut_rows, int S, XfSpec* x) {
    const int k = xf->kind & 0xff;
    if (k == TMAC_XF_NORM || k == TMAC_XF_GLU_NORM)
        return fail(TMAC_HIP_E_ARG, "experts call: %s is not served in front of an experts call (TMAC_XF_NONE or TMAC_XF_GLU)", k == TMAC_XF_NORM ? "TMAC_XF_NORM" : "TMAC_XF_GLU_NORM");
    const int32_t rc = xf_resolve(xf, XF_SITE_N1, x);
    if (rc) return rc;
    if (x->kind == TMAC_XF_GLU && lut_rows != S)
        return fail(TMAC_HIP_E_ARG, "experts call: a GLU takes one row of in and in2 per slot: lut_rows=%d, S=%d", lut_rows, S);
    return TMAC_HIP_OK;
}

extern "C" int32_t tmac_hip_debug_experts_fused_plan(int K, int bits, int group_size, const int* bank_Mw, int nbanks, int S, int lut_rows, int combine,
                                                     int32_t kind, int32_t* wpq, int32_t* grid, int32_t* items, size_t* lds_bytes) {
    alignas(16) static const char operand[16] = {};      // (a pure twin has no operands: this passes the resolver's in2 rules)
    tmac_hip_xform xf{};
    xf.kind = kind;
    xf.in2 = operand;
    XfSpec x;
    const int32_t rc = experts_xf_check(&xf, lut_rows, S, &x);
    if (rc) return rc;
    return tmac_hip_debug_experts_plan(K, bits, group_size, bank_Mw, nbanks, S, lut_rows, combine, wpq, grid, items, lds_bytes);
}

extern "C" int32_t tmac_hip_qgemm_experts_fused_dev(const tmac_hip_bank* const* banks, int nbanks, const void* B_dev, tmac_dtype_t act_dtype, int lut_rows,
                                                    const tmac_hip_xform* xf, const int32_t* ids_dev, const float* gates_dev, int S, void* const* C_dev,
                                                    tmac_dtype_t out_dtype, void* stream) {
    bind_thread_device();
    // every check before anything is launched or flushed: a refused call launches nothing and leaves the deferred queue as it is
    XfSpec x;
    if (xf) {
        const int32_t xrc = experts_xf_check(xf, lut_rows, S, &x);
        if (xrc) return xrc;
    }
    ExpertsArgs a;
    int32_t rc = experts_call_check("tmac_hip_qgemm_experts_fused_dev", banks, nbanks, B_dev, lut_rows, ids_dev, gates_dev, S, C_dev, out_dtype, a);
    if (rc) return rc;
    rc = defer_barrier();                     // never queued: behind the calling thread's queue
    if (rc) return rc;
    a.lutsrc = x.kind == TMAC_XF_GLU ? 2 : 1;
    a.B = B_dev; a.in2 = x.in2; a.act_f16 = act_dtype == TMAC_F16;
    a.xf_kind = x.kind | (x.gate << 8);
    return experts_launch(a, (hipStream_t)stream);
}

// ---- token batches: the grouped GEMM over routed positions (k_lut_image_pos + k_gemm_experts, tmac_experts_gemm.hip) ----
extern "C" int32_t tmac_hip_debug_experts_gemm_plan(int K, int bits, int group_size, const int* bank_Mw, int nbanks, int N, int S, int E, int P,
                                                    int32_t* grid_x, int32_t* grid_y, size_t* lds_bytes) {
    if (!bank_Mw) return fail(TMAC_HIP_E_ARG, "null argument");
    Shape s{};
    s.K = K; s.bits = bits; s.gs = group_size; s.ags = 64; s.m_groups = -1; s.zero_point = 1;
    set_layout(s, L_QUAD);
    ExpertsGemmPlan p;
    if (!experts_gemm_plan(s, bank_Mw, nbanks, N, S, E, P, p)) return fail(TMAC_HIP_E_NOMATCH, "experts rows call: %s", p.why);
    if (grid_x) *grid_x = p.gx;
    if (grid_y) *grid_y = p.gy;
    if (lds_bytes) *lds_bytes = p.lds_bytes;
    return TMAC_HIP_OK;
}

hipError_t tmac::launch_gemm_experts(const ExpertsGemmArgs& a_in, const ExpertsGemmPlan& p, hipStream_t st) {
    ExpertsGemmArgs a = a_in;
    if (p.why || a.nbanks < 1 || a.nbanks > EXPERTS_MAX_BANKS || a.P != 64 * p.gy) return hipErrorInvalidValue;
    for (int b = 0; b < a.nbanks; ++b) a.b[b].wg_end = p.wg_end[b];
    a.apg_shift = 0;
    while ((64 << a.apg_shift) < a.s.gs) ++a.apg_shift;
    return sel_int<1, 2, 3, 4>(a.s.bits, [&](auto BITS) { return launch_gemm_experts_unit<decltype(BITS)::value>(a, p, st); });
}

extern "C" int32_t tmac_hip_qgemm_experts_rows_dev(const tmac_hip_bank* const* banks, int nbanks, const void* B_dev, tmac_dtype_t act_dtype, int x_rows,
                                                   const int32_t* tile_expert_dev, const int32_t* src_dev, int N, int S, void* const* C_dev,
                                                   tmac_dtype_t out_dtype, void* stream) {
    bind_thread_device();
    // every check before anything is launched or flushed: a refused call launches nothing and leaves the deferred queue as it is
    if (!banks || !C_dev || nbanks < 1 || nbanks > EXPERTS_MAX_BANKS) return fail(TMAC_HIP_E_ARG, "tmac_hip_qgemm_experts_rows_dev takes one or two banks (nbanks=%d)", nbanks);
    for (int b = 0; b < nbanks; ++b)
        if (!banks[b] || !C_dev[b]) return fail(TMAC_HIP_E_ARG, "null bank or output");
    if (!B_dev || !tile_expert_dev || !src_dev) return fail(TMAC_HIP_E_ARG, "null activations or routing");
    if (chain_recording()) return fail(TMAC_HIP_E_ARG, "tmac_hip_qgemm_experts_rows_dev cannot be recorded (tmac_hip_chain_begin ... _end): expert calls run stand-alone");
    const tmac_hip_bank* b0 = banks[0];
    const Shape& s0 = b0->s;
    const int E = (int)b0->experts.size();
    if (nbanks == 2) {
        const Shape& s1 = banks[1]->s;
        if (s1.K != s0.K || s1.bits != s0.bits || s1.gs != s0.gs || s1.ags != s0.ags || s1.zero_point != s0.zero_point || banks[1]->sc_dtype != b0->sc_dtype)
            return fail(TMAC_HIP_E_ARG, "banks of one call share K, bits, group size, zero-point setting and scale dtype (their rows may differ)");
        if ((int)banks[1]->experts.size() != E) return fail(TMAC_HIP_E_ARG, "banks of one call share the routing: %d and %d experts", E, (int)banks[1]->experts.size());
    }
    ExpertsRowsSizes z;
    if (!experts_rows_sizes(N, S, E, z)) return fail(TMAC_HIP_E_ARG, "experts rows call (N=%d, S=%d, E=%d): %s", N, S, E, z.why);
    if (x_rows != N && x_rows != z.P)
        return fail(TMAC_HIP_E_ARG, "x_rows=%d: N=%d (token-major activations) or P=%d (position-major)", x_rows, N, z.P);
    for (int b = 0; b < nbanks; ++b)
        if (misaligned(C_dev[b], out_align(out_dtype)))
            return fail(TMAC_HIP_E_ARG, "C_dev[%d] must be %zu-byte aligned (four outputs are stored at a time)", b, out_align(out_dtype));
    if (misaligned(B_dev, ACT_ALIGN)) return fail(TMAC_HIP_E_ARG, "B_dev must be %zu-byte aligned (the LUT build reads 16 bytes at a time)", ACT_ALIGN);
    if (misaligned(tile_expert_dev, 4) || misaligned(src_dev, 4)) return fail(TMAC_HIP_E_ARG, "tile_expert_dev and src_dev must be 4-byte aligned");
    ExpertsGemmArgs a;
    memset(&a, 0, sizeof(a));
    int Mw[EXPERTS_MAX_BANKS] = {0, 0};
    for (int b = 0; b < nbanks; ++b) {
        Mw[b] = banks[b]->s.Mw;
        a.b[b].tab = banks[b]->tab; a.b[b].C = C_dev[b]; a.b[b].E = E; a.b[b].Mw = Mw[b];
    }
    ExpertsGemmPlan p;
    if (!experts_gemm_plan(s0, Mw, nbanks, N, S, E, z.P, p)) return fail(TMAC_HIP_E_NOMATCH, "experts rows call (K=%d, N=%d, S=%d): %s", s0.K, N, S, p.why);
    int32_t rc = defer_barrier();             // never queued: behind the calling thread's queue (B_dev may be a queued call's output)
    if (rc) return rc;
    const hipStream_t st = (hipStream_t)stream;
    tmac_hip_workspace* ws = nullptr;
    if ((rc = stream_workspace(st, s0.K, z.P, &ws)) != TMAC_HIP_OK) return rc;
    LutBuildReq q;
    q.K = s0.K; q.N = z.P; q.ags = s0.ags; q.want = LB_IMAGE;
    q.src_dev = src_dev; q.row_div = x_rows == z.P ? 0 : S; q.x_rows = x_rows;      // (P > N S >= N: the two never coincide)
    LutBuildPlan lb;
    if ((rc = lut_build_plan(q, lut_caps(ws), &lb)) != TMAC_HIP_OK) return rc;
    if ((rc = lut_build(ws, lb, B_dev, act_dtype, nullptr, nullptr, st)) != TMAC_HIP_OK) return rc;
    a.nbanks = nbanks; a.s = s0;
    a.tile_expert = tile_expert_dev; a.src = src_dev;
    a.bimg = (const uint4*)ws->gimg; a.colv = ws->gcol; a.P = z.P;
    a.sc_f16 = b0->sc_dtype == F16; a.out_f16 = out_dtype == TMAC_F16;
    const hipError_t e = launch_gemm_experts(a, p, st);
    if (e != hipSuccess) return fail(TMAC_HIP_E_RUNTIME, "experts rows kernel launch: %s", hipGetErrorString(e));
    return TMAC_HIP_OK;
}
