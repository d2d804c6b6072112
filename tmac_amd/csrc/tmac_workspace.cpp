// tmac_workspace.cpp — the LUT workspace (TMACGeMMWrapper::set_workspace, tmac_gemm_wrapper.h:257-270, on the device), the preprocessor
// entry points that fill it (lut_ctor.cc:38-266 + generated glue) through lut_build, the one caller of the LUT builders (what they leave in
// the workspace: tmac_lut_held.h), and the per-stream workspaces of the fused entry point's N >= 2 routes.
#include "tmac_host.h"

using namespace tmac_host;

extern "C" int32_t tmac_hip_workspace_create(tmac_hip_workspace** out, int maxK, int maxN) {
    if (!out || maxK <= 0 || maxN <= 0 || maxK % 64) return fail(TMAC_HIP_E_ARG, "bad workspace size (maxK must be a multiple of 64)");
    int32_t rc = ensure_device();
    if (rc) return rc;
    auto* ws = new tmac_hip_workspace();
    ws->maxK = maxK; ws->maxN = maxN;
    const size_t nq = (size_t)maxN * (maxK / 4) * 16, nd = (size_t)maxN * qdev_u4_for_K(maxK) * 16, nl = (size_t)maxN * qlut_lds_u4(maxK) * 16;
    const size_t ns = sizeof(float) * (size_t)maxN * (maxK / 32);
    hipError_t e = hipMalloc((void**)&ws->qlut_ref, nq);
    if (e == hipSuccess) e = hipMalloc(&ws->qlut_dev, nd);
    if (e == hipSuccess) e = hipMemset(ws->qlut_dev, 0x80, nd);
    if (e == hipSuccess) e = hipMalloc(&ws->qlut_lds, nl);
    if (e == hipSuccess) e = hipMemset(ws->qlut_lds, 0x80, nl);
    if (e == hipSuccess) e = hipMalloc((void**)&ws->lut_scales, ns);
    if (e == hipSuccess) e = hipMalloc((void**)&ws->lut_biases, ns);
    if (e == hipSuccess) e = hipMalloc((void**)&ws->xf_r, sizeof(float) * (size_t)maxN);
    if (maxN > 1) {
        ws->gNpad = (maxN + 63) & ~63;
        if (e == hipSuccess) e = hipMalloc(&ws->gimg, (size_t)2 * maxK * ws->gNpad);
        if (e == hipSuccess) e = hipMalloc((void**)&ws->gcol, sizeof(float) * 4 * (size_t)(maxK / 64) * ws->gNpad);
    }
    // The fills above are null-stream work and the workspace's users launch on streams of their own (the host-pointer layer
    // and the ggml glue on NON-BLOCKING streams, which the null stream does not order): a fill that lands after the first
    // LUT build leaves all-zero half tables behind (round 2: qgemm_lut_int8 returned the bias terms only).  Complete them here.
    if (e == hipSuccess && g_knobs.ws_fill_sync) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) {   // nothing of a half-built workspace is left behind
        tmac_hip_workspace_free(ws);
        return fail(TMAC_HIP_E_RUNTIME, "workspace allocation (K=%d, N=%d): %s", maxK, maxN, hipGetErrorString(e));
    }
    *out = ws;
    return TMAC_HIP_OK;
}

extern "C" int32_t tmac_hip_workspace_free(tmac_hip_workspace* ws) {
    if (!ws) return TMAC_HIP_OK;
    if (ws->qlut_ref) (void)hipFree(ws->qlut_ref);
    if (ws->qlut_dev) (void)hipFree(ws->qlut_dev);
    if (ws->qlut_lds) (void)hipFree(ws->qlut_lds);
    if (ws->lut_scales) (void)hipFree(ws->lut_scales);
    if (ws->lut_biases) (void)hipFree(ws->lut_biases);
    if (ws->xf_r) (void)hipFree(ws->xf_r);
    if (ws->gimg) (void)hipFree(ws->gimg);
    if (ws->gcol) (void)hipFree(ws->gcol);
    if (ws->dump) (void)hipFree(ws->dump);
    delete ws;
    return TMAC_HIP_OK;
}

int32_t tmac_host::check_lut_shape(tmac_hip_workspace* ws, int K, int N, int ags) {
    if (!ws) return fail(TMAC_HIP_E_ARG, "null workspace");
    return lut_shape_check(K, N, ags, ws->maxK, ws->maxN);
}

LutBuildCaps tmac_host::lut_caps(const tmac_hip_workspace* ws) {
    LutBuildCaps c;
    c.pairs_min_n = g_knobs.pairs_min_n;
    c.image_min_n = g_knobs.gemm_kernel == 1 ? INT_MAX : gemm_min_rows(PLANES_MIN_N);
    c.image_buffers = ws->gimg != nullptr;
    c.maxK = ws->maxK; c.maxN = ws->maxN;
    return c;
}

int32_t tmac_host::lut_build(tmac_hip_workspace* ws, const LutBuildPlan& plan, const void* B_dev, tmac_dtype_t act_dtype, const XfRowsGateArgs* xf,
                             const int32_t* perm_dev, hipStream_t st) {
    ws->held.clear();
    const LutHeld& h = plan.held;
    const int K = h.K(), N = h.N(), f16 = act_dtype == TMAC_F16;
    const bool all = plan.all_layouts, row_img = plan.row_image;
    int8_t* const ref = all ? ws->qlut_ref : nullptr;
    void* const dev = all ? ws->qlut_dev : nullptr;
    const size_t dev_u4 = all ? h.qdev_u4_per_row() : 0;
    hipError_t e = hipSuccess;
    switch (plan.builder) {
    case LUTB_PREPROCESS:
        e = launch_preprocess(B_dev, (Dtype)act_dtype, ws->qlut_ref, ws->qlut_dev, ws->qlut_lds, ws->lut_scales, ws->lut_biases, K, N, h.ags(), dev_u4, st);
        break;
    case LUTB_PAIRS:
        e = launch_preprocess_pairs(B_dev, f16, ws->qlut_lds, ws->lut_scales, ws->lut_biases, K, N, ref, dev, dev_u4, st, xf, perm_dev);
        break;
    case LUTB_PAIRS_ROW:
        e = launch_preprocess_pairs_row(B_dev, f16, ws->qlut_lds, ws->lut_scales, ws->lut_biases, K, N, ref, dev, dev_u4, row_img ? ws->gimg : nullptr,
                                        row_img ? ws->gcol : nullptr, all || row_img ? ws->gNpad : 0, st, xf);
        break;
    case LUTB_NONE: break;
    }
    // (a builder that writes no layout is there for its image)
    if (e != hipSuccess) return fail(TMAC_HIP_E_RUNTIME, "%s launch: %s", h.has_layout(LUT_HALF) ? "preprocess" : "LUT image", hipGetErrorString(e));
    if (plan.lut_image) {
        e = launch_lut_image(B_dev, f16, ws->gimg, ws->gcol, K, N, ws->gNpad, st, xf, perm_dev);
        if (e != hipSuccess) return fail(TMAC_HIP_E_RUNTIME, "LUT image launch: %s", hipGetErrorString(e));
    }
    ws->held.commit(plan);
    return TMAC_HIP_OK;
}

// kp: through this K permutation (act-order handles, tmac_kperm.h): every layout of the workspace from x[perm], by the gathered pair build,
// for every N; the workspace records the permutation's id, which tmac_hip_qgemm_dev holds the weights to
static int32_t preprocessor_impl(tmac_hip_workspace* ws, const void* B_dev, tmac_dtype_t act_dtype, int K, int N, int act_group_size,
                                 const KPermData* kp, hipStream_t st) {
    bind_thread_device();
    int32_t rc = defer_barrier();             // behind the calling thread's deferred queue (B_dev may be a queued call's output)
    if (rc) return rc;
    rc = check_lut_shape(ws, K, N, act_group_size);
    if (rc) return rc;
    if (!B_dev) return fail(TMAC_HIP_E_ARG, "null activations");
    if (misaligned(B_dev, ACT_ALIGN)) return fail(TMAC_HIP_E_ARG, "B_dev must be %zu-byte aligned (the LUT build reads 16 bytes at a time)", ACT_ALIGN);
    LutBuildReq q;
    q.K = K; q.N = N; q.ags = act_group_size; q.want = LB_ALL;
    if (kp) { q.perm_id = kp->h.id; q.perm_K = kp->h.K; }
    LutBuildPlan plan;
    rc = lut_build_plan(q, lut_caps(ws), &plan);
    if (rc) return rc;
    return lut_build(ws, plan, B_dev, act_dtype, nullptr, kp ? kp->dev : nullptr, st);
}

extern "C" int32_t tmac_hip_preprocessor_dev(tmac_hip_workspace* ws, const void* B_dev, tmac_dtype_t act_dtype, int K,
                                             int N, int act_group_size, void* stream) {
    return preprocessor_impl(ws, B_dev, act_dtype, K, N, act_group_size, nullptr, (hipStream_t)stream);
}

// NULL or identity: the plain call
extern "C" int32_t tmac_hip_preprocessor_perm_dev(tmac_hip_workspace* ws, const void* B_dev, tmac_dtype_t act_dtype, int K, int N, int act_group_size,
                                                  const tmac_hip_kperm* perm, void* stream) {
    const KPermData* kp = perm && perm->d && !perm->d->h.identity ? perm->d.get() : nullptr;
    return preprocessor_impl(ws, B_dev, act_dtype, K, N, act_group_size, kp, (hipStream_t)stream);
}

extern "C" int32_t tmac_hip_workspace_ptrs(tmac_hip_workspace* ws, void** qlut_dev, size_t* nbytes_qlut_per_row,
                                           void** lut_scales, void** lut_biases) {
    if (!ws) return fail(TMAC_HIP_E_ARG, "null workspace");
    if (qlut_dev) *qlut_dev = ws->qlut_dev;
    if (nbytes_qlut_per_row) *nbytes_qlut_per_row = ws->held.qdev_u4_per_row() * 16;
    if (lut_scales) *lut_scales = ws->lut_scales;
    if (lut_biases) *lut_biases = ws->lut_biases;
    return TMAC_HIP_OK;
}

extern "C" int32_t tmac_hip_workspace_read(tmac_hip_workspace* ws, int8_t* qlut_host, float* lut_scales_host,
                                           float* lut_biases_host, int K, int N, int act_group_size, void* stream) {
    int32_t rc = defer_barrier();
    if (rc) return rc;
    rc = check_lut_shape(ws, K, N, act_group_size);
    if (rc) return rc;
    if (!ws->held.holds_exactly(K, N, act_group_size)) return fail(TMAC_HIP_E_ARG, "workspace holds a different LUT");
    hipStream_t st = (hipStream_t)stream;
    const size_t G = (size_t)K / act_group_size;
    if (qlut_host) HIP_TRY(hipMemcpyAsync(qlut_host, ws->qlut_ref, (size_t)N * (K / 4) * 16, hipMemcpyDeviceToHost, st));
    if (lut_scales_host) HIP_TRY(hipMemcpyAsync(lut_scales_host, ws->lut_scales, sizeof(float) * N * G, hipMemcpyDeviceToHost, st));
    if (lut_biases_host) HIP_TRY(hipMemcpyAsync(lut_biases_host, ws->lut_biases, sizeof(float) * N * G, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return TMAC_HIP_OK;
}

extern "C" int32_t tmac_hip_workspace_write(tmac_hip_workspace* ws, const int8_t* qlut_host, const float* lut_scales_host,
                                            const float* lut_biases_host, int K, int N, int act_group_size, void* stream) {
    int32_t rc = defer_barrier();
    if (rc) return rc;
    rc = check_lut_shape(ws, K, N, act_group_size);
    if (rc) return rc;
    if (!qlut_host || !lut_scales_host || !lut_biases_host) return fail(TMAC_HIP_E_ARG, "null LUT pointer");
    hipStream_t st = (hipStream_t)stream;
    const size_t G = (size_t)K / act_group_size;
    const LutBuildPlan plan = lut_write_plan(K, N, act_group_size);      // (no image: the one there was built from activations, not from this LUT)
    ws->held.clear();
    HIP_TRY(hipMemcpyAsync(ws->qlut_ref, qlut_host, (size_t)N * (K / 4) * 16, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ws->lut_scales, lut_scales_host, sizeof(float) * N * G, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ws->lut_biases, lut_biases_host, sizeof(float) * N * G, hipMemcpyHostToDevice, st));
    hipError_t e = launch_qlut_ref_to_dev(ws->qlut_ref, ws->qlut_dev, ws->qlut_lds, K, N, plan.held.qdev_u4_per_row(), st);
    if (e != hipSuccess) return fail(TMAC_HIP_E_RUNTIME, "qlut_ref_to_dev launch: %s", hipGetErrorString(e));
    ws->held.commit(plan);
    return TMAC_HIP_OK;
}

// ---- the fused entry point's workspaces ------------------------------------------------------------------------------------------------
static std::map<std::pair<int, hipStream_t>, tmac_hip_workspace*> g_fused_ws;   // per (device, stream): the null stream exists on every device

int32_t tmac_host::stream_workspace(hipStream_t st, int K, int N, tmac_hip_workspace** out) {
    std::lock_guard<std::mutex> lk(g_mu);
    tmac_hip_workspace*& slot = g_fused_ws[std::make_pair(g_device, st)];
    int needK = K, needN = N;
    if (slot && (slot->maxK < K || slot->maxN < N)) {
        // grow to the maximum seen in BOTH dimensions (mixed shapes -- K = 4096 / 11008, growing N -- would otherwise
        // free and reallocate on every other call); the old buffers may still be read by launches in flight
        needK = slot->maxK > K ? slot->maxK : K;
        needN = slot->maxN > N ? slot->maxN : N;
        hipError_t e = hipStreamSynchronize(st);
        if (e != hipSuccess) return fail(TMAC_HIP_E_RUNTIME, "stream sync: %s", hipGetErrorString(e));
        tmac_hip_workspace_free(slot);
        slot = nullptr;
    }
    if (!slot) {
        int32_t rc = tmac_hip_workspace_create(&slot, needK, needN);
        if (rc) { slot = nullptr; return rc; }
    }
    *out = slot;
    return TMAC_HIP_OK;
}

void tmac_host::release_fused_workspaces() {
    for (auto& kv : g_fused_ws) {
        (void)hipStreamSynchronize(kv.first.second);      // launches in flight may still read the LUT workspace
        tmac_hip_workspace_free(kv.second);
    }
    g_fused_ws.clear();
}
