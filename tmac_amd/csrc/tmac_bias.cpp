// tmac_bias.cpp — the bias of a handle: y = W x + b.  The handle owns an fp32 copy of b (k_bias_copy, tmac_pack.hip), which k_gemv_quad's and
// k_gemm_planes' bias instantiations add in front of an output's one store; which calls take such a handle is tmac_dispatch.cpp's.
#include "tmac_host.h"

using namespace tmac_host;

extern "C" int32_t tmac_hip_weights_set_bias_dev(tmac_hip_weights* w, const void* bias_dev, tmac_src_dtype_t dtype, void* stream) {
    if (!w) return fail(TMAC_HIP_E_ARG, "null weights");
    if (!bias_dev) return fail(TMAC_HIP_E_ARG, "bias_dev is NULL");
    if (misaligned(bias_dev, 16)) return fail(TMAC_HIP_E_ARG, "bias_dev is not 16-byte aligned");
    if (dtype != TMAC_SRC_F32 && dtype != TMAC_SRC_F16 && dtype != TMAC_SRC_BF16)
        return fail(TMAC_HIP_E_ARG, "the bias dtype must be TMAC_SRC_F32, TMAC_SRC_F16 or TMAC_SRC_BF16");
    if (w->bias) return fail(TMAC_HIP_E_ARG, "the handle already has a bias (it is set once, straight after registration)");
    if (w->s.m_groups >= 1) return fail(TMAC_HIP_E_NOMATCH, "m_groups = %d: unified-scale handles take no bias", w->s.m_groups);
    if (w->kperm) return fail(TMAC_HIP_E_ARG, "the handle carries a K permutation (act-order): a bias on such handles is not served yet");
    // the two kernels that add a bias read the QUAD layout (whatever variant is selected when a call comes: the call's own refusal)
    if (quad_mfma_misses(w) & (QM_LAYOUT | QM_FAST_AGG | QM_SHAPE))
        return fail(TMAC_HIP_E_NOMATCH, "a bias is served on k_gemv_quad's MFMA form and k_gemm_planes only: QUAD layout, no fast aggregation, a shape k_gemv_quad takes");
    int32_t rc = ensure_device();
    if (rc) return rc;
    rc = defer_barrier();       // bias_dev may have been written by queued work
    if (rc) return rc;
    const int Mw = w->s.Mw, Mpad = (Mw + 63) & ~63;
    float* copy = nullptr;
    HIP_TRY(hipMalloc((void**)&copy, sizeof(float) * (size_t)Mpad));
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = launch_bias_copy(bias_dev, dtype, copy, Mw, Mpad, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);      // the copy is the handle's from here on, on every stream
    if (e != hipSuccess) {
        (void)hipFree(copy);
        return fail(TMAC_HIP_E_RUNTIME, "bias copy: %s", hipGetErrorString(e));
    }
    defer_forget_all();         // (recordings cached by the deferred queue name the handle as it was: without a bias)
    w->bias = copy;
    return TMAC_HIP_OK;
}

extern "C" int32_t tmac_hip_weights_has_bias(const tmac_hip_weights* w, int* has) {
    if (!w || !has) return fail(TMAC_HIP_E_ARG, "null argument");
    *has = w->bias ? 1 : 0;
    return TMAC_HIP_OK;
}
