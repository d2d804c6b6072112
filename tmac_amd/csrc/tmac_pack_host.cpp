// tmac_pack_host.cpp — the entry points in front of the pack kernels (tmac_pack.hip): GPTQ tensors or plain codes, in device memory, ->
// the reference blob (tmac_hip_pack_*_dev) or straight to a registered handle (tmac_hip_register_weights_*_dev, through register_impl).
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

int32_t launch(const Shape& s, const GptqIn& in, void* A_out, void* S_out, tmac_dtype_t ref_float, hipStream_t st) {
    const hipError_t e = launch_pack_gptq(in.qweight, in.scales, in.qzeros, (Dtype)in.scales_dtype, in.gptq_v2, A_out, S_out, (Dtype)ref_float, s, st);
    return e == hipSuccess ? TMAC_HIP_OK : fail(TMAC_HIP_E_RUNTIME, "pack_gptq: %s", hipGetErrorString(e));
}
int32_t launch(const Shape& s, const CodesIn& in, void* A_out, void* S_out, tmac_dtype_t ref_float, hipStream_t st) {
    const hipError_t e = launch_pack_codes(in.codes, in.scales, in.zeros, (Dtype)in.sz_dtype, A_out, S_out, (Dtype)ref_float, s, st);
    return e == hipSuccess ? TMAC_HIP_OK : fail(TMAC_HIP_E_RUNTIME, "pack_codes: %s", hipGetErrorString(e));
}

// pack into the caller's buffers: behind the calling thread's deferred queue like every entry point that writes caller memory
template <class In>
int32_t pack_to(const Shape& s, const In& in, void* A_out, void* S_out, tmac_dtype_t ref_float, void* stream) {
    int32_t rc = ensure_device();
    if (rc) return rc;
    rc = defer_barrier();
    if (rc) return rc;
    return launch(s, in, A_out, S_out, ref_float, (hipStream_t)stream);
}

// Pack into temporaries, register from them, free them.  register_impl uses device sources in place when it keeps no reference copy and
// copies them otherwise; either way the temporaries stay ours, and no work that names them is in flight once it has synchronised.
template <class In>
int32_t register_from(tmac_hip_weights** out, const Shape& s, const In& in, int Mw, int K, int bits, const tmac_kcfg* cfg, tmac_dtype_t ref_float,
                      tmac_dtype_t dev_float, void* stream) {
    int32_t rc = ensure_device();
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    DevBuf dA, dS;      // freed on every return path; hipFree waits for the device, so also after a failure in front of the synchronise
    HIP_TRY(dA.alloc(ref_weight_bytes(s)));
    HIP_TRY(dS.alloc(ref_scale_elems(s) * dt_size((Dtype)ref_float)));
    rc = launch(s, in, dA.p, dS.p, ref_float, st);
    if (rc == TMAC_HIP_OK) rc = register_impl(out, dA.p, dS.p, true, Mw, K, bits, cfg, ref_float, dev_float, stream);
    if (rc != TMAC_HIP_OK) (void)hipStreamSynchronize(st);
    return rc;
}

}  // namespace

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
