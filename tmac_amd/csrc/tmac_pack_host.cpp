// tmac_pack_host.cpp — the entry points in front of the pack kernels (tmac_pack.hip): GPTQ tensors or plain codes, in device memory, ->
// the reference blob (tmac_hip_pack_*_dev) or straight to a registered handle (tmac_hip_register_weights_*_dev, through register_impl).
// BitNet master weights (fp32 / fp16 / bf16) take the same two ways through the absmean rule (tmac_hip_*_absmean_dev), packed ternary
// BitNet weights (four weight rows per byte) through tmac_hip_*_ternary_dev, dense master weights to W1 - W4 with per-group scales by
// round to nearest through tmac_hip_*_rtn_dev, AutoAWQ GEMM tensors (4 bits) through tmac_hip_*_awq_dev.
#include <cmath>

#include "tmac_host.h"

using namespace tmac_host;

namespace {

constexpr size_t PACK_ALIGN = 16;      // every device pointer of these calls: the kernels load and store 16 bytes at a time

struct PackArg { const char* name; const void* p; bool required; };

// Everything that is refused before anything is written, in this order: NULL required pointers (E_ARG), the GPTQ form's widths (E_NOMATCH),
// make_shape's own refusals, the form's argument rules (E_ARG), alignment (E_ARG).
int32_t pack_check(Shape& s, bool gptq, const PackArg* args, int nargs, const void* zeros, const char* zeros_name, int dtype, const char* dtype_name,
                   int Mw, int K, int bits, const tmac_kcfg* cfg, tmac_dtype_t ref_float) {
    if (!cfg) return fail(TMAC_HIP_E_ARG, "null kcfg");
    for (int i = 0; i < nargs; ++i)
        if (args[i].required && !args[i].p) return fail(TMAC_HIP_E_ARG, "%s is NULL", args[i].name);
    if (dtype != TMAC_F32 && dtype != TMAC_F16) return fail(TMAC_HIP_E_ARG, "%s must be TMAC_F32 or TMAC_F16", dtype_name);
    if (ref_float != TMAC_F32 && ref_float != TMAC_F16) return fail(TMAC_HIP_E_ARG, "ref_float must be TMAC_F32 or TMAC_F16");
    if (gptq && bits != 1 && bits != 2 && bits != 4)
        return fail(TMAC_HIP_E_NOMATCH, "GPTQ-packed weights of width %d are not served (1, 2 and 4: fields that do not straddle a word); "
                                         "pass unpacked codes to the codes form", bits);
    int32_t rc = make_shape(s, Mw, K, bits, cfg);
    if (rc) return rc;
    if (gptq && s.m_groups >= 1) return fail(TMAC_HIP_E_ARG, "m_groups = %d: the GPTQ form has per-group scales only", s.m_groups);
    if (gptq && K % (32 / bits)) return fail(TMAC_HIP_E_NOMATCH, "K=%d is no whole number of qweight words (%d values each)", K, 32 / bits);
    if (zeros && !s.zero_point) return fail(TMAC_HIP_E_ARG, "%s given, but the configuration has no zero points (zero_point == 0)", zeros_name);
    if (!zeros && s.zero_point) return fail(TMAC_HIP_E_ARG, "%s is NULL, but the configuration has zero points (zero_point != 0)", zeros_name);
    for (int i = 0; i < nargs; ++i)
        if (args[i].p && misaligned(args[i].p, PACK_ALIGN)) return fail(TMAC_HIP_E_ARG, "%s is not %zu-byte aligned", args[i].name, PACK_ALIGN);
    return TMAC_HIP_OK;
}

struct GptqIn { const void *qweight, *scales, *qzeros; tmac_dtype_t scales_dtype; int gptq_v2; };
struct CodesIn { const void *codes, *scales, *zeros; tmac_dtype_t sz_dtype; };

int32_t check_gptq(Shape& s, const GptqIn& in, const void* A_out, const void* S_out, bool outs, int Mw, int K, int bits, const tmac_kcfg* cfg,
                   tmac_dtype_t ref_float) {
    const PackArg args[] = {{"qweight", in.qweight, true}, {"scales", in.scales, true}, {"qzeros", in.qzeros, false},
                            {"A_ref_out", A_out, outs}, {"scales_ref_out", S_out, outs}};
    return pack_check(s, true, args, 5, in.qzeros, "qzeros", in.scales_dtype, "scales_dtype", Mw, K, bits, cfg, ref_float);
}
int32_t check_codes(Shape& s, const CodesIn& in, const void* A_out, const void* S_out, bool outs, int Mw, int K, int bits, const tmac_kcfg* cfg,
                    tmac_dtype_t ref_float) {
    const PackArg args[] = {{"codes", in.codes, true}, {"scales", in.scales, true}, {"zeros", in.zeros, false},
                            {"A_ref_out", A_out, outs}, {"scales_ref_out", S_out, outs}};
    return pack_check(s, false, args, 5, in.zeros, "zeros", in.sz_dtype, "sz_dtype", Mw, K, bits, cfg, ref_float);
}

// perm: the device copy of an act-order permutation (every value < K), or null
int32_t launch(const Shape& s, const GptqIn& in, void* A_out, void* S_out, tmac_dtype_t ref_float, hipStream_t st, const int32_t* perm = nullptr) {
    const hipError_t e = launch_pack_gptq(in.qweight, in.scales, in.qzeros, (Dtype)in.scales_dtype, in.gptq_v2, A_out, S_out, (Dtype)ref_float, s, st, perm);
    return e == hipSuccess ? TMAC_HIP_OK : fail(TMAC_HIP_E_RUNTIME, "pack_gptq: %s", hipGetErrorString(e));
}
int32_t launch(const Shape& s, const CodesIn& in, void* A_out, void* S_out, tmac_dtype_t ref_float, hipStream_t st, const int32_t* perm = nullptr) {
    const hipError_t e = launch_pack_codes(in.codes, in.scales, in.zeros, (Dtype)in.sz_dtype, A_out, S_out, (Dtype)ref_float, s, st, perm);
    return e == hipSuccess ? TMAC_HIP_OK : fail(TMAC_HIP_E_RUNTIME, "pack_codes: %s", hipGetErrorString(e));
}

// ---- AutoAWQ (the format: tmac_pack.h) ---------------------------------------------------------------------------------------------------
struct AwqIn { const void *qweight, *scales, *qzeros; tmac_dtype_t scales_dtype; };

// pack_check's rules for the codes form (NULL pointers, dtypes, make_shape's refusals, zeros against zero_point, alignment) and the format's
// own: 4 bits, per-group scales
int32_t check_awq(Shape& s, const AwqIn& in, const void* A_out, const void* S_out, bool outs, int Mw, int K, const tmac_kcfg* cfg, tmac_dtype_t ref_float) {
    const PackArg args[] = {{"qweight", in.qweight, true}, {"scales", in.scales, true}, {"qzeros", in.qzeros, false},
                            {"A_ref_out", A_out, outs}, {"scales_ref_out", S_out, outs}};
    // the width a configuration describes is bm * n_tile_num / Mw (n_tile_num <= 0: not filled in, nothing to contradict)
    if (cfg && cfg->n_tile_num > 0 && (long long)cfg->bm * cfg->n_tile_num != 4ll * Mw)
        return fail(TMAC_HIP_E_ARG, "AWQ is packed at 4 bits: the configuration (bm=%d x n_tile_num=%d) does not describe Mw=%d rows of 4 bits", cfg->bm,
                    cfg->n_tile_num, Mw);
    const int32_t rc = pack_check(s, false, args, 5, in.qzeros, "qzeros", in.scales_dtype, "scales_dtype", Mw, K, 4, cfg, ref_float);
    if (rc) return rc;
    if (s.m_groups >= 1) return fail(TMAC_HIP_E_ARG, "m_groups = %d: the AWQ form has per-group scales only", s.m_groups);
    return TMAC_HIP_OK;
}

int32_t launch(const Shape& s, const AwqIn& in, void* A_out, void* S_out, tmac_dtype_t ref_float, hipStream_t st, const int32_t* = nullptr) {
    const hipError_t e = launch_pack_awq(in.qweight, in.scales, in.qzeros, (Dtype)in.scales_dtype, A_out, S_out, (Dtype)ref_float, s, st);
    return e == hipSuccess ? TMAC_HIP_OK : fail(TMAC_HIP_E_RUNTIME, "pack_awq: %s", hipGetErrorString(e));
}

// pack into the caller's buffers: behind the calling thread's deferred queue like every entry point that writes caller memory
template <class In>
int32_t pack_to(const Shape& s, const In& in, void* A_out, void* S_out, tmac_dtype_t ref_float, void* stream, const int32_t* perm = nullptr) {
    int32_t rc = ensure_device();
    if (rc) return rc;
    rc = defer_barrier();
    if (rc) return rc;
    return launch(s, in, A_out, S_out, ref_float, (hipStream_t)stream, perm);
}

// Pack into temporaries, register from them, free them.  register_impl uses device sources in place when it keeps no reference copy and
// copies them otherwise; either way the temporaries stay ours, and no work that names them is in flight once it has synchronised.
// kperm (act-order): the pack reads through it, and the new handle shares its ownership.
template <class In>
int32_t register_from(tmac_hip_weights** out, const Shape& s, const In& in, int Mw, int K, int bits, const tmac_kcfg* cfg, tmac_dtype_t ref_float,
                      tmac_dtype_t dev_float, void* stream, const std::shared_ptr<KPermData>& kperm = nullptr) {
    int32_t rc = ensure_device();
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    DevBuf dA, dS;      // freed on every return path; hipFree waits for the device, so also after a failure in front of the synchronise
    HIP_TRY(dA.alloc(ref_weight_bytes(s)));
    HIP_TRY(dS.alloc(ref_scale_elems(s) * dt_size((Dtype)ref_float)));
    rc = launch(s, in, dA.p, dS.p, ref_float, st, kperm ? kperm->dev : nullptr);
    if (rc == TMAC_HIP_OK) rc = register_impl(out, dA.p, dS.p, true, Mw, K, bits, cfg, ref_float, dev_float, stream);
    if (rc != TMAC_HIP_OK) (void)hipStreamSynchronize(st);
    else (*out)->kperm = kperm;
    return rc;
}

// What a permuted pack adds to the argument rules of its plain twin: per-group scales, and the permutation's K and group size are the
// call's.  (A null or identity permutation never gets here: the plain twin is called.)
int32_t check_perm(const Shape& s, const tmac_hip_kperm* perm) {
    if (s.m_groups >= 1) return fail(TMAC_HIP_E_ARG, "m_groups = %d: unified-scale weights take no K permutation", s.m_groups);
    const KPermHost& h = perm->d->h;
    if (h.K != s.K || h.gs != s.gs)
        return fail(TMAC_HIP_E_ARG, "the K permutation was built for K=%d, group_size=%d; the call has K=%d, group_size=%d", h.K, h.gs, s.K, s.gs);
    return TMAC_HIP_OK;
}
bool perm_is_plain(const tmac_hip_kperm* perm) { return !perm || !perm->d || perm->d->h.identity; }

// ---- BitNet master weights (the absmean rule: tmac_pack.h) -------------------------------------------------------------------------------
struct DenseIn { const void* W; int src; const float* scales_in; float eps; };

// The argument rules the three entry points share, in front of any shape rule: NULL required pointers, the source dtype, eps, the row
// blocks.  (m_groups is the call's own argument for the reduction alone and cfg->m_groups otherwise.)
int32_t masters_check(const PackArg* args, int nargs, int src_dtype, float eps, int Mw, int m_groups) {
    for (int i = 0; i < nargs; ++i)
        if (args[i].required && !args[i].p) return fail(TMAC_HIP_E_ARG, "%s is NULL", args[i].name);
    if (src_dtype != TMAC_SRC_F32 && src_dtype != TMAC_SRC_F16 && src_dtype != TMAC_SRC_BF16)
        return fail(TMAC_HIP_E_ARG, "src_dtype must be TMAC_SRC_F32, TMAC_SRC_F16 or TMAC_SRC_BF16");
    if (!std::isfinite(eps) || !(eps > 0.0f)) return fail(TMAC_HIP_E_ARG, "eps must be finite and > 0");
    if (m_groups < 1) return fail(TMAC_HIP_E_ARG, "m_groups = %d: master weights take unified scales (per-group scales: register codes or GPTQ tensors)", m_groups);
    if (Mw % m_groups) return fail(TMAC_HIP_E_ARG, "Mw=%d is no whole number of m_groups=%d row blocks", Mw, m_groups);
    return TMAC_HIP_OK;
}
int32_t aligned_check(const PackArg* args, int nargs) {
    for (int i = 0; i < nargs; ++i)
        if (args[i].p && misaligned(args[i].p, PACK_ALIGN)) return fail(TMAC_HIP_E_ARG, "%s is not %zu-byte aligned", args[i].name, PACK_ALIGN);
    return TMAC_HIP_OK;
}
// ... and of the two that pack: the rules above, then make_shape's own refusals (bits = 2), then alignment
int32_t check_dense(Shape& s, const DenseIn& in, const void* A_out, const void* S_out, bool outs, int Mw, int K, const tmac_kcfg* cfg, tmac_dtype_t ref_float) {
    if (!cfg) return fail(TMAC_HIP_E_ARG, "null kcfg");
    const PackArg args[] = {{"W_dev", in.W, true}, {"scales_in_dev", in.scales_in, false}, {"A_ref_out", A_out, outs}, {"scales_ref_out", S_out, outs}};
    int32_t rc = masters_check(args, 4, in.src, in.eps, Mw, cfg->m_groups);
    if (rc) return rc;
    if (ref_float != TMAC_F32 && ref_float != TMAC_F16) return fail(TMAC_HIP_E_ARG, "host_float must be TMAC_F32 or TMAC_F16");
    rc = make_shape(s, Mw, K, 2, cfg);
    return rc ? rc : aligned_check(args, 4);
}

// The launches: the reduction into scratch of our own unless the caller brought the scales, then the pack.  With a computed scale the
// stream is waited for before the scratch goes.
int32_t launch(const Shape& s, const DenseIn& in, void* A_out, void* S_out, tmac_dtype_t ref_float, hipStream_t st) {
    const float* scales = in.scales_in;
    DevBuf scratch;     // [partials: doubles][scales: m_groups floats]
    hipError_t e = hipSuccess;
    if (!scales) {
        const size_t np = absmean_partial_count(s.Mw, s.K, s.m_groups);
        HIP_TRY(scratch.alloc(sizeof(double) * np + sizeof(float) * (size_t)s.m_groups));
        float* sc = reinterpret_cast<float*>(scratch.as<double>() + np);
        e = launch_absmean(in.W, in.src, s.Mw, s.K, s.m_groups, in.eps, scratch.as<double>(), sc, st);
        scales = sc;
    }
    if (e == hipSuccess) e = launch_pack_dense(in.W, in.src, scales, A_out, S_out, (Dtype)ref_float, s, st);
    if (e != hipSuccess) return fail(TMAC_HIP_E_RUNTIME, "pack_absmean: %s", hipGetErrorString(e));
    if (scratch.p) HIP_TRY(hipStreamSynchronize(st));
    return TMAC_HIP_OK;
}

// ---- BitNet packed ternary checkpoints (the format: tmac_pack.h) ---------------------------------------------------------------------------
struct TernaryIn { const void* packed; const float* scales; };

// Everything that is refused before anything is written, in the order of check_dense: NULL required pointers, the row blocks, the blob's
// dtype, make_shape's own refusals (bits = 2), alignment -- of the counter too, where one is given.
int32_t check_ternary(Shape& s, const TernaryIn& in, const void* A_out, const void* S_out, bool outs, const int32_t* invalid, int Mw, int K, const tmac_kcfg* cfg,
                      tmac_dtype_t ref_float) {
    if (!cfg) return fail(TMAC_HIP_E_ARG, "null kcfg");
    const PackArg args[] = {{"packed_dev", in.packed, true}, {"scales_dev", in.scales, true}, {"A_ref_out", A_out, outs}, {"scales_ref_out", S_out, outs},
                            {"invalid_count_dev", invalid, false}};
    for (const PackArg& a : args)
        if (a.required && !a.p) return fail(TMAC_HIP_E_ARG, "%s is NULL", a.name);
    if (cfg->m_groups < 1)
        return fail(TMAC_HIP_E_ARG, "m_groups = %d: packed ternary weights take unified scales (per-group scales: register codes or GPTQ tensors)", cfg->m_groups);
    if (Mw % cfg->m_groups) return fail(TMAC_HIP_E_ARG, "Mw=%d is no whole number of m_groups=%d row blocks", Mw, cfg->m_groups);
    if (ref_float != TMAC_F32 && ref_float != TMAC_F16) return fail(TMAC_HIP_E_ARG, "host_float must be TMAC_F32 or TMAC_F16");
    const int32_t rc = make_shape(s, Mw, K, 2, cfg);
    return rc ? rc : aligned_check(args, 5);
}

// the counter zeroed on the stream, then the pack
int32_t launch(const Shape& s, const TernaryIn& in, void* A_out, void* S_out, tmac_dtype_t ref_float, int32_t* invalid, hipStream_t st) {
    if (invalid) HIP_TRY(hipMemsetAsync(invalid, 0, sizeof(int32_t), st));
    const hipError_t e = launch_pack_ternary(in.packed, in.scales, A_out, S_out, (Dtype)ref_float, s, invalid, g_knobs.pack_ternary_kernel == 1, st);
    return e == hipSuccess ? TMAC_HIP_OK : fail(TMAC_HIP_E_RUNTIME, "pack_ternary: %s", hipGetErrorString(e));
}

}  // namespace

extern "C" int32_t tmac_hip_debug_pack_ternary_kernel(int mode) {
    if (mode < 0 || mode > 1) return fail(TMAC_HIP_E_ARG, "packed ternary kernel mode must be 0 (auto: read-once where it applies) or 1 (the general form everywhere)");
    g_knobs.pack_ternary_kernel = mode;
    return TMAC_HIP_OK;
}

extern "C" int32_t tmac_hip_pack_ternary_dev(const void* packed_dev, const float* scales_dev, int Mw, int K, const tmac_kcfg* cfg, void* A_ref_out,
                                             void* scales_ref_out, tmac_dtype_t host_float, int32_t* invalid_count_dev, void* stream) {
    const TernaryIn in{packed_dev, scales_dev};
    Shape s;
    int32_t rc = check_ternary(s, in, A_ref_out, scales_ref_out, true, invalid_count_dev, Mw, K, cfg, host_float);
    if (rc) return rc;
    rc = ensure_device();
    if (rc) return rc;
    rc = defer_barrier();
    return rc ? rc : launch(s, in, A_ref_out, scales_ref_out, host_float, invalid_count_dev, (hipStream_t)stream);
}

extern "C" int32_t tmac_hip_register_weights_ternary_dev(tmac_hip_weights** out, const void* packed_dev, const float* scales_dev, int Mw, int K,
                                                         const tmac_kcfg* cfg, tmac_dtype_t host_float, tmac_dtype_t dev_float, void* stream) {
    if (!out) return fail(TMAC_HIP_E_ARG, "out is NULL");
    const TernaryIn in{packed_dev, scales_dev};
    Shape s;
    int32_t rc = check_ternary(s, in, nullptr, nullptr, false, nullptr, Mw, K, cfg, host_float);
    if (rc) return rc;
    if (dev_float != TMAC_F32 && dev_float != TMAC_F16) return fail(TMAC_HIP_E_ARG, "dev_float must be TMAC_F32 or TMAC_F16");
    rc = ensure_device();
    if (rc) return rc;
    rc = defer_barrier();       // packed_dev / scales_dev may have been written by queued work
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    DevBuf dA, dS, dN;  // as register_from: ours on every return path
    HIP_TRY(dA.alloc(ref_weight_bytes(s)));
    HIP_TRY(dS.alloc(ref_scale_elems(s) * dt_size((Dtype)host_float)));
    HIP_TRY(dN.alloc(sizeof(int32_t)));
    rc = launch(s, in, dA.p, dS.p, host_float, dN.as<int32_t>(), st);
    if (rc != TMAC_HIP_OK) {
        (void)hipStreamSynchronize(st);
        return rc;
    }
    int32_t invalid = 0;
    HIP_TRY(hipMemcpyAsync(&invalid, dN.p, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (invalid) return fail(TMAC_HIP_E_ARG, "packed weight holds %d fields of value 3 (no ternary level)", invalid);
    rc = register_impl(out, dA.p, dS.p, true, Mw, K, 2, cfg, host_float, dev_float, stream);
    if (rc != TMAC_HIP_OK) (void)hipStreamSynchronize(st);
    return rc;
}

extern "C" int32_t tmac_hip_absmean_dev(const void* W_dev, tmac_src_dtype_t src_dtype, int Mw, int K, int m_groups, float eps, float* scales_out_dev,
                                        void* stream) {
    const PackArg args[] = {{"W_dev", W_dev, true}, {"scales_out_dev", scales_out_dev, true}};
    int32_t rc = masters_check(args, 2, src_dtype, eps, Mw, m_groups);
    if (rc) return rc;
    if (Mw <= 0 || K <= 0 || K % 4) return fail(TMAC_HIP_E_ARG, "Mw=%d and K=%d must be positive, K a multiple of 4", Mw, K);
    rc = aligned_check(args, 2);
    if (rc) return rc;
    rc = ensure_device();
    if (rc) return rc;
    rc = defer_barrier();
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    DevBuf partials;
    HIP_TRY(partials.alloc(sizeof(double) * absmean_partial_count(Mw, K, m_groups)));
    const hipError_t e = launch_absmean(W_dev, src_dtype, Mw, K, m_groups, eps, partials.as<double>(), scales_out_dev, st);
    if (e != hipSuccess) return fail(TMAC_HIP_E_RUNTIME, "absmean: %s", hipGetErrorString(e));
    HIP_TRY(hipStreamSynchronize(st));      // the scratch goes with this call
    return TMAC_HIP_OK;
}

extern "C" int32_t tmac_hip_pack_absmean_dev(const void* W_dev, tmac_src_dtype_t src_dtype, const float* scales_in_dev, float eps, int Mw, int K,
                                             const tmac_kcfg* cfg, void* A_ref_out, void* scales_ref_out, tmac_dtype_t host_float, void* stream) {
    const DenseIn in{W_dev, src_dtype, scales_in_dev, eps};
    Shape s;
    int32_t rc = check_dense(s, in, A_ref_out, scales_ref_out, true, Mw, K, cfg, host_float);
    if (rc) return rc;
    rc = ensure_device();
    if (rc) return rc;
    rc = defer_barrier();
    return rc ? rc : launch(s, in, A_ref_out, scales_ref_out, host_float, (hipStream_t)stream);
}

extern "C" int32_t tmac_hip_register_weights_absmean_dev(tmac_hip_weights** out, const void* W_dev, tmac_src_dtype_t src_dtype, const float* scales_in_dev,
                                                         float eps, int Mw, int K, const tmac_kcfg* cfg, tmac_dtype_t host_float, tmac_dtype_t dev_float,
                                                         void* stream) {
    if (!out) return fail(TMAC_HIP_E_ARG, "out is NULL");
    const DenseIn in{W_dev, src_dtype, scales_in_dev, eps};
    Shape s;
    int32_t rc = check_dense(s, in, nullptr, nullptr, false, Mw, K, cfg, host_float);
    if (rc) return rc;
    rc = ensure_device();
    if (rc) return rc;
    rc = defer_barrier();       // W_dev / scales_in_dev may have been written by queued work
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    DevBuf dA, dS;      // as register_from: ours on every return path
    HIP_TRY(dA.alloc(ref_weight_bytes(s)));
    HIP_TRY(dS.alloc(ref_scale_elems(s) * dt_size((Dtype)host_float)));
    rc = launch(s, in, dA.p, dS.p, host_float, st);
    if (rc == TMAC_HIP_OK) rc = register_impl(out, dA.p, dS.p, true, Mw, K, 2, cfg, host_float, dev_float, stream);
    if (rc != TMAC_HIP_OK) (void)hipStreamSynchronize(st);
    return rc;
}

// ---- dense master weights -> W1 - W4 with per-group scales: round to nearest (the rule: tmac_pack.h) ---------------------------------------
namespace {

struct RtnIn { const void* W; int src; };

int32_t src_dtype_check(int src_dtype) {
    if (src_dtype != TMAC_SRC_F32 && src_dtype != TMAC_SRC_F16 && src_dtype != TMAC_SRC_BF16)
        return fail(TMAC_HIP_E_ARG, "src_dtype must be TMAC_SRC_F32, TMAC_SRC_F16 or TMAC_SRC_BF16");
    return TMAC_HIP_OK;
}

// Everything that is refused before anything is written, in the order of check_dense: NULL required pointers, the source dtype, the scales'
// form, the blob's dtype, make_shape's own refusals, alignment -- of the counter too, where one is given.
int32_t check_rtn(Shape& s, const RtnIn& in, const void* A_out, const void* S_out, bool outs, const int32_t* invalid, int Mw, int K, int bits,
                  const tmac_kcfg* cfg, tmac_dtype_t ref_float) {
    if (!cfg) return fail(TMAC_HIP_E_ARG, "null kcfg");
    const PackArg args[] = {{"W_dev", in.W, true}, {"A_ref_out", A_out, outs}, {"scales_ref_out", S_out, outs}, {"invalid_count_dev", invalid, false}};
    for (const PackArg& a : args)
        if (a.required && !a.p) return fail(TMAC_HIP_E_ARG, "%s is NULL", a.name);
    int32_t rc = src_dtype_check(in.src);
    if (rc) return rc;
    if (cfg->m_groups >= 1)
        return fail(TMAC_HIP_E_ARG, "m_groups = %d: round to nearest gives per-group scales (unified scales from master weights: "
                                    "tmac_hip_register_weights_absmean_dev)", cfg->m_groups);
    if (ref_float != TMAC_F32 && ref_float != TMAC_F16) return fail(TMAC_HIP_E_ARG, "host_float must be TMAC_F32 or TMAC_F16");
    rc = make_shape(s, Mw, K, bits, cfg);
    return rc ? rc : aligned_check(args, 4);
}

// The launches: the parameters of every (row, group) into scratch of our own, the counter zeroed on the stream in front of them, then the
// pack.  The stream is waited for before the scratch goes.
int32_t launch(const Shape& s, const RtnIn& in, int scale_f16, void* A_out, void* S_out, tmac_dtype_t ref_float, int32_t* invalid, hipStream_t st) {
    const size_t items = (size_t)s.Mw * (s.K / s.gs);
    DevBuf params;      // [scales][zq][zeros]: fp32 [Mw][K / gs] each
    HIP_TRY(params.alloc(sizeof(float) * items * 3));
    float *sc = params.as<float>(), *zq = sc + items, *zr = s.zero_point ? zq + items : nullptr;
    if (invalid) HIP_TRY(hipMemsetAsync(invalid, 0, sizeof(int32_t), st));
    hipError_t e = launch_rtn_params(in.W, in.src, s.Mw, s.K, s.bits, s.gs, s.zero_point, scale_f16, sc, zq, zr, invalid, st);
    if (e == hipSuccess) e = launch_pack_rtn(in.W, in.src, sc, zq, zr, A_out, S_out, (Dtype)ref_float, s, st);
    if (e != hipSuccess) return fail(TMAC_HIP_E_RUNTIME, "pack_rtn: %s", hipGetErrorString(e));
    HIP_TRY(hipStreamSynchronize(st));
    return TMAC_HIP_OK;
}

}  // namespace

extern "C" int32_t tmac_hip_rtn_params_dev(const void* W_dev, tmac_src_dtype_t src_dtype, int Mw, int K, int bits, int group_size, int zero_point,
                                           int scale_f16, float* scales_out_dev, float* zq_out_dev, int32_t* invalid_count_dev, void* stream) {
    const PackArg args[] = {{"W_dev", W_dev, true}, {"scales_out_dev", scales_out_dev, true}, {"zq_out_dev", zq_out_dev, true},
                            {"invalid_count_dev", invalid_count_dev, false}};
    for (const PackArg& a : args)
        if (a.required && !a.p) return fail(TMAC_HIP_E_ARG, "%s is NULL", a.name);
    int32_t rc = src_dtype_check(src_dtype);
    if (rc) return rc;
    if (bits < 1 || bits > 4) return fail(TMAC_HIP_E_ARG, "bits=%d: 1 to 4 are served", bits);
    if (Mw <= 0 || K <= 0 || group_size <= 0 || group_size % 4 || K % group_size)
        return fail(TMAC_HIP_E_ARG, "Mw=%d, K=%d and group_size=%d must be positive, group_size a multiple of 4 that divides K", Mw, K, group_size);
    rc = aligned_check(args, 4);
    if (rc) return rc;
    rc = ensure_device();
    if (rc) return rc;
    rc = defer_barrier();
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (invalid_count_dev) HIP_TRY(hipMemsetAsync(invalid_count_dev, 0, sizeof(int32_t), st));
    const hipError_t e = launch_rtn_params(W_dev, src_dtype, Mw, K, bits, group_size, zero_point, scale_f16, scales_out_dev, zq_out_dev, nullptr,
                                           invalid_count_dev, st);
    return e == hipSuccess ? TMAC_HIP_OK : fail(TMAC_HIP_E_RUNTIME, "rtn_params: %s", hipGetErrorString(e));
}

extern "C" int32_t tmac_hip_pack_rtn_dev(const void* W_dev, tmac_src_dtype_t src_dtype, int Mw, int K, int bits, const tmac_kcfg* cfg, void* A_ref_out,
                                         void* scales_ref_out, tmac_dtype_t host_float, int32_t* invalid_count_dev, void* stream) {
    const RtnIn in{W_dev, src_dtype};
    Shape s;
    int32_t rc = check_rtn(s, in, A_ref_out, scales_ref_out, true, invalid_count_dev, Mw, K, bits, cfg, host_float);
    if (rc) return rc;
    rc = ensure_device();
    if (rc) return rc;
    rc = defer_barrier();
    return rc ? rc : launch(s, in, host_float == TMAC_F16, A_ref_out, scales_ref_out, host_float, invalid_count_dev, (hipStream_t)stream);
}

extern "C" int32_t tmac_hip_register_weights_rtn_dev(tmac_hip_weights** out, const void* W_dev, tmac_src_dtype_t src_dtype, int Mw, int K, int bits,
                                                     const tmac_kcfg* cfg, tmac_dtype_t host_float, tmac_dtype_t dev_float, void* stream) {
    if (!out) return fail(TMAC_HIP_E_ARG, "out is NULL");
    const RtnIn in{W_dev, src_dtype};
    Shape s;
    int32_t rc = check_rtn(s, in, nullptr, nullptr, false, nullptr, Mw, K, bits, cfg, host_float);
    if (rc) return rc;
    if (dev_float != TMAC_F32 && dev_float != TMAC_F16) return fail(TMAC_HIP_E_ARG, "dev_float must be TMAC_F32 or TMAC_F16");
    rc = ensure_device();
    if (rc) return rc;
    rc = defer_barrier();       // W_dev may have been written by queued work
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    DevBuf dA, dS, dN;  // as register_from: ours on every return path
    HIP_TRY(dA.alloc(ref_weight_bytes(s)));
    HIP_TRY(dS.alloc(ref_scale_elems(s) * dt_size((Dtype)host_float)));
    HIP_TRY(dN.alloc(sizeof(int32_t)));
    // the scale that divides is the scale the handle stores: rounded to fp16 up front wherever the blob or the handle keeps fp16 scales
    rc = launch(s, in, host_float == TMAC_F16 || dev_float == TMAC_F16, dA.p, dS.p, host_float, dN.as<int32_t>(), st);
    if (rc != TMAC_HIP_OK) {
        (void)hipStreamSynchronize(st);
        return rc;
    }
    int32_t invalid = 0;
    HIP_TRY(hipMemcpyAsync(&invalid, dN.p, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (invalid)
        return fail(TMAC_HIP_E_ARG, "master weights hold %d groups that cannot be quantised (a master that is not finite, or a scale that is 0 or "
                                    "not finite in the scales' dtype)", invalid);
    rc = register_impl(out, dA.p, dS.p, true, Mw, K, bits, cfg, host_float, dev_float, stream);
    if (rc != TMAC_HIP_OK) (void)hipStreamSynchronize(st);
    return rc;
}

// ---- the K permutation object (tmac_kperm.h: the rules; here: the device copies and the lifetime) -----------------------------------------
extern "C" int32_t tmac_hip_kperm_from_gidx_dev(const int32_t* g_idx_dev, int K, int group_size, tmac_hip_kperm** out, void* stream) {
    if (!out) return fail(TMAC_HIP_E_ARG, "out is NULL");
    if (!g_idx_dev) return fail(TMAC_HIP_E_ARG, "g_idx_dev is NULL");
    if (misaligned(g_idx_dev, PACK_ALIGN)) return fail(TMAC_HIP_E_ARG, "g_idx_dev is not %zu-byte aligned", PACK_ALIGN);
    if (K <= 0 || group_size <= 0) return fail(TMAC_HIP_E_ARG, "g_idx: K=%d and group_size=%d must be positive", K, group_size);
    int32_t rc = ensure_device();
    if (rc) return rc;
    rc = defer_barrier();       // g_idx_dev may have been written by queued work
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    std::vector<int32_t> g((size_t)K);
    HIP_TRY(hipMemcpyAsync(g.data(), g_idx_dev, sizeof(int32_t) * (size_t)K, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    auto d = std::make_shared<KPermData>();
    rc = kperm_build(g.data(), K, group_size, &d->h);
    if (rc) return rc;
    HIP_TRY(hipMalloc((void**)&d->dev, sizeof(int32_t) * (size_t)K));
    HIP_TRY(hipMemcpyAsync(d->dev, d->h.perm.data(), sizeof(int32_t) * (size_t)K, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));      // the host copy is pageable: done before anyone can free the object
    *out = new tmac_hip_kperm{std::move(d)};
    return TMAC_HIP_OK;
}

extern "C" int32_t tmac_hip_kperm_info(const tmac_hip_kperm* p, int* K, int* identity, uint64_t* id) {
    if (!p || !p->d) return fail(TMAC_HIP_E_ARG, "null permutation");
    if (K) *K = p->d->h.K;
    if (identity) *identity = p->d->h.identity ? 1 : 0;
    if (id) *id = p->d->h.id;
    return TMAC_HIP_OK;
}

extern "C" int32_t tmac_hip_kperm_read(const tmac_hip_kperm* p, int32_t* perm_host) {
    if (!p || !p->d || !perm_host) return fail(TMAC_HIP_E_ARG, "null argument");
    memcpy(perm_host, p->d->h.perm.data(), sizeof(int32_t) * (size_t)p->d->h.K);
    return TMAC_HIP_OK;
}

extern "C" int32_t tmac_hip_kperm_free(tmac_hip_kperm* p) {
    delete p;       // the data lives on while a handle registered through it does
    return TMAC_HIP_OK;
}

// ---- packing and registration through a permutation: the plain twins' argument lists plus `perm`; null or identity calls the twin --------
extern "C" int32_t tmac_hip_pack_gptq_perm_dev(const void* qweight, const void* scales, const void* qzeros, tmac_dtype_t scales_dtype, int gptq_v2,
                                               const tmac_hip_kperm* perm, int Mw, int K, int bits, const tmac_kcfg* cfg, void* A_ref_out,
                                               void* scales_ref_out, tmac_dtype_t ref_float, void* stream) {
    if (perm_is_plain(perm))
        return tmac_hip_pack_gptq_dev(qweight, scales, qzeros, scales_dtype, gptq_v2, Mw, K, bits, cfg, A_ref_out, scales_ref_out, ref_float, stream);
    const GptqIn in{qweight, scales, qzeros, scales_dtype, gptq_v2};
    Shape s;
    int32_t rc = check_gptq(s, in, A_ref_out, scales_ref_out, true, Mw, K, bits, cfg, ref_float);
    if (rc == TMAC_HIP_OK) rc = check_perm(s, perm);
    return rc ? rc : pack_to(s, in, A_ref_out, scales_ref_out, ref_float, stream, perm->d->dev);
}

extern "C" int32_t tmac_hip_pack_codes_perm_dev(const void* codes, const void* scales, const void* zeros, tmac_dtype_t sz_dtype,
                                                const tmac_hip_kperm* perm, int Mw, int K, int bits, const tmac_kcfg* cfg, void* A_ref_out,
                                                void* scales_ref_out, tmac_dtype_t ref_float, void* stream) {
    if (perm_is_plain(perm)) return tmac_hip_pack_codes_dev(codes, scales, zeros, sz_dtype, Mw, K, bits, cfg, A_ref_out, scales_ref_out, ref_float, stream);
    const CodesIn in{codes, scales, zeros, sz_dtype};
    Shape s;
    int32_t rc = check_codes(s, in, A_ref_out, scales_ref_out, true, Mw, K, bits, cfg, ref_float);
    if (rc == TMAC_HIP_OK) rc = check_perm(s, perm);
    return rc ? rc : pack_to(s, in, A_ref_out, scales_ref_out, ref_float, stream, perm->d->dev);
}

extern "C" int32_t tmac_hip_register_weights_gptq_perm_dev(tmac_hip_weights** out, const void* qweight, const void* scales, const void* qzeros,
                                                           tmac_dtype_t scales_dtype, int gptq_v2, const tmac_hip_kperm* perm, int Mw, int K, int bits,
                                                           const tmac_kcfg* cfg, tmac_dtype_t ref_float, tmac_dtype_t dev_float, void* stream) {
    if (perm_is_plain(perm))
        return tmac_hip_register_weights_gptq_dev(out, qweight, scales, qzeros, scales_dtype, gptq_v2, Mw, K, bits, cfg, ref_float, dev_float, stream);
    if (!out) return fail(TMAC_HIP_E_ARG, "out is NULL");
    const GptqIn in{qweight, scales, qzeros, scales_dtype, gptq_v2};
    Shape s;
    int32_t rc = check_gptq(s, in, nullptr, nullptr, false, Mw, K, bits, cfg, ref_float);
    if (rc == TMAC_HIP_OK) rc = check_perm(s, perm);
    return rc ? rc : register_from(out, s, in, Mw, K, bits, cfg, ref_float, dev_float, stream, perm->d);
}

extern "C" int32_t tmac_hip_register_weights_codes_perm_dev(tmac_hip_weights** out, const void* codes, const void* scales, const void* zeros,
                                                            tmac_dtype_t sz_dtype, const tmac_hip_kperm* perm, int Mw, int K, int bits,
                                                            const tmac_kcfg* cfg, tmac_dtype_t ref_float, tmac_dtype_t dev_float, void* stream) {
    if (perm_is_plain(perm))
        return tmac_hip_register_weights_codes_dev(out, codes, scales, zeros, sz_dtype, Mw, K, bits, cfg, ref_float, dev_float, stream);
    if (!out) return fail(TMAC_HIP_E_ARG, "out is NULL");
    const CodesIn in{codes, scales, zeros, sz_dtype};
    Shape s;
    int32_t rc = check_codes(s, in, nullptr, nullptr, false, Mw, K, bits, cfg, ref_float);
    if (rc == TMAC_HIP_OK) rc = check_perm(s, perm);
    return rc ? rc : register_from(out, s, in, Mw, K, bits, cfg, ref_float, dev_float, stream, perm->d);
}

extern "C" int32_t tmac_hip_weights_kperm_id(const tmac_hip_weights* w, uint64_t* id) {
    if (!w || !id) return fail(TMAC_HIP_E_ARG, "null argument");
    *id = w->kperm ? w->kperm->h.id : 0;
    return TMAC_HIP_OK;
}

extern "C" int32_t tmac_hip_ref_blob_bytes(int Mw, int K, int bits, const tmac_kcfg* cfg, tmac_dtype_t ref_float, size_t* a_bytes, size_t* s_bytes) {
    if (ref_float != TMAC_F32 && ref_float != TMAC_F16) return fail(TMAC_HIP_E_ARG, "ref_float must be TMAC_F32 or TMAC_F16");
    Shape s;
    const int32_t rc = make_shape(s, Mw, K, bits, cfg);
    if (rc) return rc;
    if (a_bytes) *a_bytes = ref_weight_bytes(s);
    if (s_bytes) *s_bytes = ref_scale_elems(s) * dt_size((Dtype)ref_float);
    return TMAC_HIP_OK;
}

extern "C" int32_t tmac_hip_pack_gptq_dev(const void* qweight, const void* scales, const void* qzeros, tmac_dtype_t scales_dtype, int gptq_v2, int Mw,
                                          int K, int bits, const tmac_kcfg* cfg, void* A_ref_out, void* scales_ref_out, tmac_dtype_t ref_float,
                                          void* stream) {
    const GptqIn in{qweight, scales, qzeros, scales_dtype, gptq_v2};
    Shape s;
    const int32_t rc = check_gptq(s, in, A_ref_out, scales_ref_out, true, Mw, K, bits, cfg, ref_float);
    return rc ? rc : pack_to(s, in, A_ref_out, scales_ref_out, ref_float, stream);
}

extern "C" int32_t tmac_hip_pack_codes_dev(const void* codes, const void* scales, const void* zeros, tmac_dtype_t sz_dtype, int Mw, int K, int bits,
                                           const tmac_kcfg* cfg, void* A_ref_out, void* scales_ref_out, tmac_dtype_t ref_float, void* stream) {
    const CodesIn in{codes, scales, zeros, sz_dtype};
    Shape s;
    const int32_t rc = check_codes(s, in, A_ref_out, scales_ref_out, true, Mw, K, bits, cfg, ref_float);
    return rc ? rc : pack_to(s, in, A_ref_out, scales_ref_out, ref_float, stream);
}

extern "C" int32_t tmac_hip_register_weights_gptq_dev(tmac_hip_weights** out, const void* qweight, const void* scales, const void* qzeros,
                                                      tmac_dtype_t scales_dtype, int gptq_v2, int Mw, int K, int bits, const tmac_kcfg* cfg,
                                                      tmac_dtype_t ref_float, tmac_dtype_t dev_float, void* stream) {
    if (!out) return fail(TMAC_HIP_E_ARG, "out is NULL");
    const GptqIn in{qweight, scales, qzeros, scales_dtype, gptq_v2};
    Shape s;
    const int32_t rc = check_gptq(s, in, nullptr, nullptr, false, Mw, K, bits, cfg, ref_float);
    return rc ? rc : register_from(out, s, in, Mw, K, bits, cfg, ref_float, dev_float, stream);
}

extern "C" int32_t tmac_hip_register_weights_codes_dev(tmac_hip_weights** out, const void* codes, const void* scales, const void* zeros,
                                                       tmac_dtype_t sz_dtype, int Mw, int K, int bits, const tmac_kcfg* cfg, tmac_dtype_t ref_float,
                                                       tmac_dtype_t dev_float, void* stream) {
    if (!out) return fail(TMAC_HIP_E_ARG, "out is NULL");
    const CodesIn in{codes, scales, zeros, sz_dtype};
    Shape s;
    const int32_t rc = check_codes(s, in, nullptr, nullptr, false, Mw, K, bits, cfg, ref_float);
    return rc ? rc : register_from(out, s, in, Mw, K, bits, cfg, ref_float, dev_float, stream);
}

// ---- AutoAWQ ---------------------------------------------------------------------------------------------------------------------------
extern "C" int32_t tmac_hip_pack_awq_dev(const void* qweight, const void* scales, const void* qzeros, tmac_dtype_t scales_dtype, int Mw, int K,
                                         const tmac_kcfg* cfg, void* A_ref_out, void* scales_ref_out, tmac_dtype_t ref_float, void* stream) {
    const AwqIn in{qweight, scales, qzeros, scales_dtype};
    Shape s;
    const int32_t rc = check_awq(s, in, A_ref_out, scales_ref_out, true, Mw, K, cfg, ref_float);
    return rc ? rc : pack_to(s, in, A_ref_out, scales_ref_out, ref_float, stream);
}

extern "C" int32_t tmac_hip_register_weights_awq_dev(tmac_hip_weights** out, const void* qweight, const void* scales, const void* qzeros,
                                                     tmac_dtype_t scales_dtype, int Mw, int K, const tmac_kcfg* cfg, tmac_dtype_t ref_float,
                                                     tmac_dtype_t dev_float, void* stream) {
    if (!out) return fail(TMAC_HIP_E_ARG, "out is NULL");
    const AwqIn in{qweight, scales, qzeros, scales_dtype};
    Shape s;
    int32_t rc = check_awq(s, in, nullptr, nullptr, false, Mw, K, cfg, ref_float);
    if (rc) return rc;
    if (dev_float != TMAC_F32 && dev_float != TMAC_F16) return fail(TMAC_HIP_E_ARG, "dev_float must be TMAC_F32 or TMAC_F16");
    rc = ensure_device();
    if (rc) return rc;
    rc = defer_barrier();       // the three tensors may have been written by queued work
    return rc ? rc : register_from(out, s, in, Mw, K, 4, cfg, ref_float, dev_float, stream);
}
