// tmac_pack_host.cpp — the entry points in front of the pack kernels (tmac_pack.hip): checkpoint tensors in device memory -> the reference
// blob (tmac_hip_pack_*_dev) or straight to a registered handle (tmac_hip_register_weights_*_dev, through register_impl).  Six formats:
// GPTQ tensors, plain codes (both also through a K permutation), AutoAWQ GEMM tensors (4 bits), BitNet master weights by the absmean
// rule, packed ternary BitNet weights (four weight rows per byte), dense master weights to W1 - W4 by round to nearest.  A format is a
// struct of its inputs with its argument rules (check) and its launches (launch); pack_to and register_from are the one route of all.
#include <cmath>

#include "tmac_host.h"

using namespace tmac_host;

namespace {

#define RC_TRY(expr)                        \
    do {                                    \
        const int32_t rc_ = (expr);         \
        if (rc_) return rc_;                \
    } while (0)

constexpr size_t PACK_ALIGN = 16;      // every device pointer of these calls: the kernels load and store 16 bytes at a time

// ---- the argument rules, once each; the names that go into the messages are the caller's ---------------------------------------------------
struct PackArg { const char* name; const void* p; bool required; };

template <size_t N> int32_t null_check(const PackArg (&args)[N]) {
    for (const PackArg& a : args)
        if (a.required && !a.p) return fail(TMAC_HIP_E_ARG, "%s is NULL", a.name);
    return TMAC_HIP_OK;
}
template <size_t N> int32_t aligned_check(const PackArg (&args)[N]) {
    for (const PackArg& a : args)
        if (a.p && misaligned(a.p, PACK_ALIGN)) return fail(TMAC_HIP_E_ARG, "%s is not %zu-byte aligned", a.name, PACK_ALIGN);
    return TMAC_HIP_OK;
}
int32_t float_dtype_check(int dtype, const char* name) {
    return dtype == TMAC_F32 || dtype == TMAC_F16 ? TMAC_HIP_OK : fail(TMAC_HIP_E_ARG, "%s must be TMAC_F32 or TMAC_F16", name);
}
int32_t src_dtype_check(int src_dtype) {
    if (src_dtype != TMAC_SRC_F32 && src_dtype != TMAC_SRC_F16 && src_dtype != TMAC_SRC_BF16)
        return fail(TMAC_HIP_E_ARG, "src_dtype must be TMAC_SRC_F32, TMAC_SRC_F16 or TMAC_SRC_BF16");
    return TMAC_HIP_OK;
}
// the two forms of scales: per-group only (why: the form's sentence), or unified only (what: the weights' name) in whole row blocks
int32_t per_group_only(int m_groups, const char* why) {
    return m_groups >= 1 ? fail(TMAC_HIP_E_ARG, "m_groups = %d: %s", m_groups, why) : TMAC_HIP_OK;
}
int32_t unified_only(int Mw, int m_groups, const char* what) {
    if (m_groups < 1) return fail(TMAC_HIP_E_ARG, "m_groups = %d: %s take unified scales (per-group scales: register codes or GPTQ tensors)", m_groups, what);
    if (Mw % m_groups) return fail(TMAC_HIP_E_ARG, "Mw=%d is no whole number of m_groups=%d row blocks", Mw, m_groups);
    return TMAC_HIP_OK;
}
// what master weights are refused for in front of any shape rule: NULL required pointers, the source dtype, eps, the row blocks
template <size_t N> int32_t masters_check(const PackArg (&args)[N], int src_dtype, float eps, int Mw, int m_groups) {
    RC_TRY(null_check(args));
    RC_TRY(src_dtype_check(src_dtype));
    if (!std::isfinite(eps) || !(eps > 0.0f)) return fail(TMAC_HIP_E_ARG, "eps must be finite and > 0");
    return unified_only(Mw, m_groups, "master weights");
}
int32_t launched(hipError_t e, const char* what) {
    return e == hipSuccess ? TMAC_HIP_OK : fail(TMAC_HIP_E_RUNTIME, "%s: %s", what, hipGetErrorString(e));
}

// ---- a call as its door hands it to the route ------------------------------------------------------------------------------------------------
struct Call {
    int Mw, K, bits;
    const tmac_kcfg* cfg;       // (never null inside a format's check)
    void *A_out, *S_out;        // the pack doors: the caller's blob, both required; the register doors: null
    bool outs;
    tmac_dtype_t ref_float;
    int32_t* invalid;           // the pack doors of a format that counts: the caller's counter, or null
};
Call packing(int Mw, int K, int bits, const tmac_kcfg* cfg, void* A_out, void* S_out, tmac_dtype_t ref_float, int32_t* invalid = nullptr) {
    return {Mw, K, bits, cfg, A_out, S_out, true, ref_float, invalid};
}
Call registering(int Mw, int K, int bits, const tmac_kcfg* cfg, tmac_dtype_t ref_float) { return {Mw, K, bits, cfg, nullptr, nullptr, false, ref_float, nullptr}; }

// What a launch may be handed beside its inputs: the device copy of an act-order permutation (every value < K; GPTQ and codes), the
// counter of items that cannot be packed (ternary, RTN: zeroed on the stream by the launch), and whether the scale that divides is rounded
// to fp16 up front (RTN: wherever the blob or the handle keeps fp16 scales, the scale that divides is the scale that is stored).
struct Extras { const int32_t* perm; int32_t* invalid; int scale_f16; };

// ---- the formats: inputs; check -- everything that is refused before anything is written, in the door's order, giving the Shape; launch;
// and, where the format counts items it cannot pack, the two halves of register's refusal around the count ----------------------------------

// The rules GPTQ, codes and AWQ share, in this order: NULL required pointers (E_ARG), the two float dtypes, the GPTQ form's widths
// (E_NOMATCH), make_shape's own refusals, the GPTQ form's argument rules, zeros against zero_point (E_ARG), alignment (E_ARG).
template <size_t N>
int32_t quant_check(Shape& s, const Call& c, const PackArg (&args)[N], bool gptq, const void* zeros, const char* zeros_name, int dtype, const char* dtype_name) {
    RC_TRY(null_check(args));
    RC_TRY(float_dtype_check(dtype, dtype_name));
    RC_TRY(float_dtype_check(c.ref_float, "ref_float"));
    if (gptq && c.bits != 1 && c.bits != 2 && c.bits != 4)
        return fail(TMAC_HIP_E_NOMATCH, "GPTQ-packed weights of width %d are not served (1, 2 and 4: fields that do not straddle a word); "
                                         "pass unpacked codes to the codes form", c.bits);
    RC_TRY(make_shape(s, c.Mw, c.K, c.bits, c.cfg));
    if (gptq) RC_TRY(per_group_only(s.m_groups, "the GPTQ form has per-group scales only"));
    if (gptq && c.K % (32 / c.bits)) return fail(TMAC_HIP_E_NOMATCH, "K=%d is no whole number of qweight words (%d values each)", c.K, 32 / c.bits);
    if (zeros && !s.zero_point) return fail(TMAC_HIP_E_ARG, "%s given, but the configuration has no zero points (zero_point == 0)", zeros_name);
    if (!zeros && s.zero_point) return fail(TMAC_HIP_E_ARG, "%s is NULL, but the configuration has zero points (zero_point != 0)", zeros_name);
    return aligned_check(args);
}

struct GptqIn {
    const void *qweight, *scales, *qzeros; tmac_dtype_t scales_dtype; int gptq_v2;
    static constexpr const char *invalid_head = nullptr, *invalid_tail = nullptr;
    int32_t check(Shape& s, const Call& c) const {
        const PackArg args[] = {{"qweight", qweight, true}, {"scales", scales, true}, {"qzeros", qzeros, false},
                                {"A_ref_out", c.A_out, c.outs}, {"scales_ref_out", c.S_out, c.outs}};
        return quant_check(s, c, args, true, qzeros, "qzeros", scales_dtype, "scales_dtype");
    }
    int32_t launch(const Shape& s, void* A_out, void* S_out, tmac_dtype_t ref_float, hipStream_t st, const Extras& x) const {
        return launched(launch_pack_gptq(qweight, scales, qzeros, (Dtype)scales_dtype, gptq_v2, A_out, S_out, (Dtype)ref_float, s, st, x.perm), "pack_gptq");
    }
};

struct CodesIn {
    const void *codes, *scales, *zeros; tmac_dtype_t sz_dtype;
    static constexpr const char *invalid_head = nullptr, *invalid_tail = nullptr;
    int32_t check(Shape& s, const Call& c) const {
        const PackArg args[] = {{"codes", codes, true}, {"scales", scales, true}, {"zeros", zeros, false},
                                {"A_ref_out", c.A_out, c.outs}, {"scales_ref_out", c.S_out, c.outs}};
        return quant_check(s, c, args, false, zeros, "zeros", sz_dtype, "sz_dtype");
    }
    int32_t launch(const Shape& s, void* A_out, void* S_out, tmac_dtype_t ref_float, hipStream_t st, const Extras& x) const {
        return launched(launch_pack_codes(codes, scales, zeros, (Dtype)sz_dtype, A_out, S_out, (Dtype)ref_float, s, st, x.perm), "pack_codes");
    }
};

// AutoAWQ (the format: tmac_pack.h): the rules of the codes form between the format's own -- 4 bits in front, per-group scales behind
struct AwqIn {
    const void *qweight, *scales, *qzeros; tmac_dtype_t scales_dtype;
    static constexpr const char *invalid_head = nullptr, *invalid_tail = nullptr;
    int32_t check(Shape& s, const Call& c) const {
        const PackArg args[] = {{"qweight", qweight, true}, {"scales", scales, true}, {"qzeros", qzeros, false},
                                {"A_ref_out", c.A_out, c.outs}, {"scales_ref_out", c.S_out, c.outs}};
        // the width a configuration describes is bm * n_tile_num / Mw (n_tile_num <= 0: not filled in, nothing to contradict)
        if (c.cfg->n_tile_num > 0 && (long long)c.cfg->bm * c.cfg->n_tile_num != 4ll * c.Mw)
            return fail(TMAC_HIP_E_ARG, "AWQ is packed at 4 bits: the configuration (bm=%d x n_tile_num=%d) does not describe Mw=%d rows of 4 bits",
                        c.cfg->bm, c.cfg->n_tile_num, c.Mw);
        RC_TRY(quant_check(s, c, args, false, qzeros, "qzeros", scales_dtype, "scales_dtype"));
        return per_group_only(s.m_groups, "the AWQ form has per-group scales only");
    }
    int32_t launch(const Shape& s, void* A_out, void* S_out, tmac_dtype_t ref_float, hipStream_t st, const Extras&) const {
        return launched(launch_pack_awq(qweight, scales, qzeros, (Dtype)scales_dtype, A_out, S_out, (Dtype)ref_float, s, st), "pack_awq");
    }
};

// BitNet master weights (the absmean rule: tmac_pack.h): masters_check, the blob's dtype, make_shape's own refusals (bits = 2), alignment
struct DenseIn {
    const void* W; int src; const float* scales_in; float eps;
    static constexpr const char *invalid_head = nullptr, *invalid_tail = nullptr;
    int32_t check(Shape& s, const Call& c) const {
        const PackArg args[] = {{"W_dev", W, true}, {"scales_in_dev", scales_in, false}, {"A_ref_out", c.A_out, c.outs}, {"scales_ref_out", c.S_out, c.outs}};
        RC_TRY(masters_check(args, src, eps, c.Mw, c.cfg->m_groups));
        RC_TRY(float_dtype_check(c.ref_float, "host_float"));
        RC_TRY(make_shape(s, c.Mw, c.K, c.bits, c.cfg));
        return aligned_check(args);
    }
    // The reduction into scratch of our own unless the caller brought the scales, then the pack.  With a computed scale the stream is
    // waited for before the scratch goes.
    int32_t launch(const Shape& s, void* A_out, void* S_out, tmac_dtype_t ref_float, hipStream_t st, const Extras&) const {
        const float* scales = scales_in;
        DevBuf scratch;     // [partials: doubles][scales: m_groups floats]
        hipError_t e = hipSuccess;
        if (!scales) {
            const size_t np = absmean_partial_count(s.Mw, s.K, s.m_groups);
            HIP_TRY(scratch.alloc(sizeof(double) * np + sizeof(float) * (size_t)s.m_groups));
            float* sc = reinterpret_cast<float*>(scratch.as<double>() + np);
            e = launch_absmean(W, src, s.Mw, s.K, s.m_groups, eps, scratch.as<double>(), sc, st);
            scales = sc;
        }
        if (e == hipSuccess) e = launch_pack_dense(W, src, scales, A_out, S_out, (Dtype)ref_float, s, st);
        RC_TRY(launched(e, "pack_absmean"));
        if (scratch.p) HIP_TRY(hipStreamSynchronize(st));
        return TMAC_HIP_OK;
    }
};

// BitNet packed ternary checkpoints (the format: tmac_pack.h), in the order of DenseIn: NULL required pointers, the row blocks, the blob's
// dtype, make_shape's own refusals (bits = 2), alignment -- of the counter too, where one is given
struct TernaryIn {
    const void* packed; const float* scales;
    static constexpr const char *invalid_head = "packed weight holds", *invalid_tail = "fields of value 3 (no ternary level)";
    int32_t check(Shape& s, const Call& c) const {
        const PackArg args[] = {{"packed_dev", packed, true}, {"scales_dev", scales, true}, {"A_ref_out", c.A_out, c.outs},
                                {"scales_ref_out", c.S_out, c.outs}, {"invalid_count_dev", c.invalid, false}};
        RC_TRY(null_check(args));
        RC_TRY(unified_only(c.Mw, c.cfg->m_groups, "packed ternary weights"));
        RC_TRY(float_dtype_check(c.ref_float, "host_float"));
        RC_TRY(make_shape(s, c.Mw, c.K, c.bits, c.cfg));
        return aligned_check(args);
    }
    int32_t launch(const Shape& s, void* A_out, void* S_out, tmac_dtype_t ref_float, hipStream_t st, const Extras& x) const {
        if (x.invalid) HIP_TRY(hipMemsetAsync(x.invalid, 0, sizeof(int32_t), st));
        return launched(launch_pack_ternary(packed, scales, A_out, S_out, (Dtype)ref_float, s, x.invalid, g_knobs.pack_ternary_kernel == 1, st), "pack_ternary");
    }
};

// Dense master weights -> W1 - W4 with per-group scales: round to nearest (the rule: tmac_pack.h), in the order of DenseIn: NULL required
// pointers, the source dtype, the scales' form, the blob's dtype, make_shape's own refusals, alignment -- of the counter too
struct RtnIn {
    const void* W; int src;
    static constexpr const char *invalid_head = "master weights hold",
                                *invalid_tail = "groups that cannot be quantised (a master that is not finite, or a scale that is 0 or not finite in the scales' dtype)";
    int32_t check(Shape& s, const Call& c) const {
        const PackArg args[] = {{"W_dev", W, true}, {"A_ref_out", c.A_out, c.outs}, {"scales_ref_out", c.S_out, c.outs}, {"invalid_count_dev", c.invalid, false}};
        RC_TRY(null_check(args));
        RC_TRY(src_dtype_check(src));
        RC_TRY(per_group_only(c.cfg->m_groups, "round to nearest gives per-group scales (unified scales from master weights: "
                                               "tmac_hip_register_weights_absmean_dev)"));
        RC_TRY(float_dtype_check(c.ref_float, "host_float"));
        RC_TRY(make_shape(s, c.Mw, c.K, c.bits, c.cfg));
        return aligned_check(args);
    }
    // The parameters of every (row, group) into scratch of our own, then the pack.  The stream is waited for before the scratch goes.
    int32_t launch(const Shape& s, void* A_out, void* S_out, tmac_dtype_t ref_float, hipStream_t st, const Extras& x) const {
        const size_t items = (size_t)s.Mw * (s.K / s.gs);
        DevBuf params;      // [scales][zq][zeros]: fp32 [Mw][K / gs] each
        HIP_TRY(params.alloc(sizeof(float) * items * 3));
        float *sc = params.as<float>(), *zq = sc + items, *zr = s.zero_point ? zq + items : nullptr;
        if (x.invalid) HIP_TRY(hipMemsetAsync(x.invalid, 0, sizeof(int32_t), st));
        hipError_t e = launch_rtn_params(W, src, s.Mw, s.K, s.bits, s.gs, s.zero_point, x.scale_f16, sc, zq, zr, x.invalid, st);
        if (e == hipSuccess) e = launch_pack_rtn(W, src, sc, zq, zr, A_out, S_out, (Dtype)ref_float, s, st);
        RC_TRY(launched(e, "pack_rtn"));
        HIP_TRY(hipStreamSynchronize(st));
        return TMAC_HIP_OK;
    }
};

// ---- the route --------------------------------------------------------------------------------------------------------------------------
// A null or identity permutation is none.  What one adds to the argument rules: per-group scales, and its K and group size are the call's.
const tmac_hip_kperm* permuting(const tmac_hip_kperm* perm) { return perm && perm->d && !perm->d->h.identity ? perm : nullptr; }

template <class In>
int32_t check_call(Shape& s, const In& in, const Call& c, const tmac_hip_kperm* perm) {
    if (!c.cfg) return fail(TMAC_HIP_E_ARG, "null kcfg");
    RC_TRY(in.check(s, c));
    if (!perm) return TMAC_HIP_OK;
    RC_TRY(per_group_only(s.m_groups, "unified-scale weights take no K permutation"));
    const KPermHost& h = perm->d->h;
    if (h.K != s.K || h.gs != s.gs)
        return fail(TMAC_HIP_E_ARG, "the K permutation was built for K=%d, group_size=%d; the call has K=%d, group_size=%d", h.K, h.gs, s.K, s.gs);
    return TMAC_HIP_OK;
}

// Pack into the caller's buffers: behind the calling thread's deferred queue like every entry point that writes caller memory.
template <class In>
int32_t pack_to(const In& in, const Call& c, void* stream, const tmac_hip_kperm* perm = nullptr) {
    perm = permuting(perm);
    Shape s;
    RC_TRY(check_call(s, in, c, perm));
    RC_TRY(ensure_device());
    RC_TRY(defer_barrier());
    return in.launch(s, c.A_out, c.S_out, c.ref_float, (hipStream_t)stream, Extras{perm ? perm->d->dev : nullptr, c.invalid, c.ref_float == TMAC_F16});
}

// Pack into temporaries, register from them, free them: behind the deferred queue as well, the inputs may have been written by queued
// work.  register_impl uses device sources in place when it keeps no reference copy and copies them otherwise; either way the
// temporaries stay ours, and no work that names them is in flight once it has synchronised.  A format that counts what it cannot pack
// has the count read back in front of register_impl, and a non-zero one refused.  perm (act-order): the pack reads through it, and the
// new handle shares its ownership.
template <class In>
int32_t register_from(tmac_hip_weights** out, const In& in, const Call& c, tmac_dtype_t dev_float, void* stream, const tmac_hip_kperm* perm = nullptr) {
    if (!out) return fail(TMAC_HIP_E_ARG, "out is NULL");
    perm = permuting(perm);
    Shape s;
    RC_TRY(check_call(s, in, c, perm));
    RC_TRY(float_dtype_check(dev_float, "dev_float"));
    RC_TRY(ensure_device());
    RC_TRY(defer_barrier());
    hipStream_t st = (hipStream_t)stream;
    DevBuf dA, dS, dN;  // freed on every return path; hipFree waits for the device, so also after a failure in front of the synchronise
    HIP_TRY(dA.alloc(ref_weight_bytes(s)));
    HIP_TRY(dS.alloc(ref_scale_elems(s) * dt_size((Dtype)c.ref_float)));
    if (In::invalid_head) HIP_TRY(dN.alloc(sizeof(int32_t)));
    int32_t rc = in.launch(s, dA.p, dS.p, c.ref_float, st, Extras{perm ? perm->d->dev : nullptr, dN.as<int32_t>(), c.ref_float == TMAC_F16 || dev_float == TMAC_F16});
    if (rc == TMAC_HIP_OK && dN.p) {
        int32_t invalid = 0;
        HIP_TRY(hipMemcpyAsync(&invalid, dN.p, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (invalid) return fail(TMAC_HIP_E_ARG, "%s %d %s", In::invalid_head, invalid, In::invalid_tail);
    }
    if (rc == TMAC_HIP_OK) rc = register_impl(out, dA.p, dS.p, true, c.Mw, c.K, c.bits, c.cfg, c.ref_float, dev_float, stream);
    if (rc != TMAC_HIP_OK) (void)hipStreamSynchronize(st);
    else if (perm) (*out)->kperm = perm->d;
    return rc;
}

}  // namespace

// ---- the doors: fill the format's inputs and the call, take the route ------------------------------------------------------------------------
extern "C" int32_t tmac_hip_pack_gptq_perm_dev(const void* qweight, const void* scales, const void* qzeros, tmac_dtype_t scales_dtype, int gptq_v2,
                                               const tmac_hip_kperm* perm, int Mw, int K, int bits, const tmac_kcfg* cfg, void* A_ref_out,
                                               void* scales_ref_out, tmac_dtype_t ref_float, void* stream) {
    return pack_to(GptqIn{qweight, scales, qzeros, scales_dtype, gptq_v2}, packing(Mw, K, bits, cfg, A_ref_out, scales_ref_out, ref_float), stream, perm);
}

extern "C" int32_t tmac_hip_pack_gptq_dev(const void* qweight, const void* scales, const void* qzeros, tmac_dtype_t scales_dtype, int gptq_v2, int Mw,
                                          int K, int bits, const tmac_kcfg* cfg, void* A_ref_out, void* scales_ref_out, tmac_dtype_t ref_float,
                                          void* stream) {
    return pack_to(GptqIn{qweight, scales, qzeros, scales_dtype, gptq_v2}, packing(Mw, K, bits, cfg, A_ref_out, scales_ref_out, ref_float), stream);
}

extern "C" int32_t tmac_hip_register_weights_gptq_perm_dev(tmac_hip_weights** out, const void* qweight, const void* scales, const void* qzeros,
                                                           tmac_dtype_t scales_dtype, int gptq_v2, const tmac_hip_kperm* perm, int Mw, int K, int bits,
                                                           const tmac_kcfg* cfg, tmac_dtype_t ref_float, tmac_dtype_t dev_float, void* stream) {
    return register_from(out, GptqIn{qweight, scales, qzeros, scales_dtype, gptq_v2}, registering(Mw, K, bits, cfg, ref_float), dev_float, stream, perm);
}

extern "C" int32_t tmac_hip_register_weights_gptq_dev(tmac_hip_weights** out, const void* qweight, const void* scales, const void* qzeros,
                                                      tmac_dtype_t scales_dtype, int gptq_v2, int Mw, int K, int bits, const tmac_kcfg* cfg,
                                                      tmac_dtype_t ref_float, tmac_dtype_t dev_float, void* stream) {
    return register_from(out, GptqIn{qweight, scales, qzeros, scales_dtype, gptq_v2}, registering(Mw, K, bits, cfg, ref_float), dev_float, stream);
}

extern "C" int32_t tmac_hip_pack_codes_perm_dev(const void* codes, const void* scales, const void* zeros, tmac_dtype_t sz_dtype,
                                                const tmac_hip_kperm* perm, int Mw, int K, int bits, const tmac_kcfg* cfg, void* A_ref_out,
                                                void* scales_ref_out, tmac_dtype_t ref_float, void* stream) {
    return pack_to(CodesIn{codes, scales, zeros, sz_dtype}, packing(Mw, K, bits, cfg, A_ref_out, scales_ref_out, ref_float), stream, perm);
}

extern "C" int32_t tmac_hip_pack_codes_dev(const void* codes, const void* scales, const void* zeros, tmac_dtype_t sz_dtype, int Mw, int K, int bits,
                                           const tmac_kcfg* cfg, void* A_ref_out, void* scales_ref_out, tmac_dtype_t ref_float, void* stream) {
    return pack_to(CodesIn{codes, scales, zeros, sz_dtype}, packing(Mw, K, bits, cfg, A_ref_out, scales_ref_out, ref_float), stream);
}

extern "C" int32_t tmac_hip_register_weights_codes_perm_dev(tmac_hip_weights** out, const void* codes, const void* scales, const void* zeros,
                                                            tmac_dtype_t sz_dtype, const tmac_hip_kperm* perm, int Mw, int K, int bits,
                                                            const tmac_kcfg* cfg, tmac_dtype_t ref_float, tmac_dtype_t dev_float, void* stream) {
    return register_from(out, CodesIn{codes, scales, zeros, sz_dtype}, registering(Mw, K, bits, cfg, ref_float), dev_float, stream, perm);
}

extern "C" int32_t tmac_hip_register_weights_codes_dev(tmac_hip_weights** out, const void* codes, const void* scales, const void* zeros,
                                                       tmac_dtype_t sz_dtype, int Mw, int K, int bits, const tmac_kcfg* cfg, tmac_dtype_t ref_float,
                                                       tmac_dtype_t dev_float, void* stream) {
    return register_from(out, CodesIn{codes, scales, zeros, sz_dtype}, registering(Mw, K, bits, cfg, ref_float), dev_float, stream);
}

extern "C" int32_t tmac_hip_pack_awq_dev(const void* qweight, const void* scales, const void* qzeros, tmac_dtype_t scales_dtype, int Mw, int K,
                                         const tmac_kcfg* cfg, void* A_ref_out, void* scales_ref_out, tmac_dtype_t ref_float, void* stream) {
    return pack_to(AwqIn{qweight, scales, qzeros, scales_dtype}, packing(Mw, K, 4, cfg, A_ref_out, scales_ref_out, ref_float), stream);
}

extern "C" int32_t tmac_hip_register_weights_awq_dev(tmac_hip_weights** out, const void* qweight, const void* scales, const void* qzeros,
                                                     tmac_dtype_t scales_dtype, int Mw, int K, const tmac_kcfg* cfg, tmac_dtype_t ref_float,
                                                     tmac_dtype_t dev_float, void* stream) {
    return register_from(out, AwqIn{qweight, scales, qzeros, scales_dtype}, registering(Mw, K, 4, cfg, ref_float), dev_float, stream);
}

extern "C" int32_t tmac_hip_pack_absmean_dev(const void* W_dev, tmac_src_dtype_t src_dtype, const float* scales_in_dev, float eps, int Mw, int K,
                                             const tmac_kcfg* cfg, void* A_ref_out, void* scales_ref_out, tmac_dtype_t host_float, void* stream) {
    return pack_to(DenseIn{W_dev, src_dtype, scales_in_dev, eps}, packing(Mw, K, 2, cfg, A_ref_out, scales_ref_out, host_float), stream);
}

extern "C" int32_t tmac_hip_register_weights_absmean_dev(tmac_hip_weights** out, const void* W_dev, tmac_src_dtype_t src_dtype, const float* scales_in_dev,
                                                         float eps, int Mw, int K, const tmac_kcfg* cfg, tmac_dtype_t host_float, tmac_dtype_t dev_float,
                                                         void* stream) {
    return register_from(out, DenseIn{W_dev, src_dtype, scales_in_dev, eps}, registering(Mw, K, 2, cfg, host_float), dev_float, stream);
}

extern "C" int32_t tmac_hip_pack_ternary_dev(const void* packed_dev, const float* scales_dev, int Mw, int K, const tmac_kcfg* cfg, void* A_ref_out,
                                             void* scales_ref_out, tmac_dtype_t host_float, int32_t* invalid_count_dev, void* stream) {
    return pack_to(TernaryIn{packed_dev, scales_dev}, packing(Mw, K, 2, cfg, A_ref_out, scales_ref_out, host_float, invalid_count_dev), stream);
}

extern "C" int32_t tmac_hip_register_weights_ternary_dev(tmac_hip_weights** out, const void* packed_dev, const float* scales_dev, int Mw, int K,
                                                         const tmac_kcfg* cfg, tmac_dtype_t host_float, tmac_dtype_t dev_float, void* stream) {
    return register_from(out, TernaryIn{packed_dev, scales_dev}, registering(Mw, K, 2, cfg, host_float), dev_float, stream);
}

extern "C" int32_t tmac_hip_pack_rtn_dev(const void* W_dev, tmac_src_dtype_t src_dtype, int Mw, int K, int bits, const tmac_kcfg* cfg, void* A_ref_out,
                                         void* scales_ref_out, tmac_dtype_t host_float, int32_t* invalid_count_dev, void* stream) {
    return pack_to(RtnIn{W_dev, src_dtype}, packing(Mw, K, bits, cfg, A_ref_out, scales_ref_out, host_float, invalid_count_dev), stream);
}

extern "C" int32_t tmac_hip_register_weights_rtn_dev(tmac_hip_weights** out, const void* W_dev, tmac_src_dtype_t src_dtype, int Mw, int K, int bits,
                                                     const tmac_kcfg* cfg, tmac_dtype_t host_float, tmac_dtype_t dev_float, void* stream) {
    return register_from(out, RtnIn{W_dev, src_dtype}, registering(Mw, K, bits, cfg, host_float), dev_float, stream);
}

extern "C" int32_t tmac_hip_debug_pack_ternary_kernel(int mode) {
    if (mode < 0 || mode > 1) return fail(TMAC_HIP_E_ARG, "packed ternary kernel mode must be 0 (auto: read-once where it applies) or 1 (the general form everywhere)");
    g_knobs.pack_ternary_kernel = mode;
    return TMAC_HIP_OK;
}

// ---- the two that pack nothing: the absmean scales and the round-to-nearest parameters alone ---------------------------------------------
extern "C" int32_t tmac_hip_absmean_dev(const void* W_dev, tmac_src_dtype_t src_dtype, int Mw, int K, int m_groups, float eps, float* scales_out_dev,
                                        void* stream) {
    const PackArg args[] = {{"W_dev", W_dev, true}, {"scales_out_dev", scales_out_dev, true}};
    RC_TRY(masters_check(args, src_dtype, eps, Mw, m_groups));
    if (Mw <= 0 || K <= 0 || K % 4) return fail(TMAC_HIP_E_ARG, "Mw=%d and K=%d must be positive, K a multiple of 4", Mw, K);
    RC_TRY(aligned_check(args));
    RC_TRY(ensure_device());
    RC_TRY(defer_barrier());
    hipStream_t st = (hipStream_t)stream;
    DevBuf partials;
    HIP_TRY(partials.alloc(sizeof(double) * absmean_partial_count(Mw, K, m_groups)));
    RC_TRY(launched(launch_absmean(W_dev, src_dtype, Mw, K, m_groups, eps, partials.as<double>(), scales_out_dev, st), "absmean"));
    HIP_TRY(hipStreamSynchronize(st));      // the scratch goes with this call
    return TMAC_HIP_OK;
}

extern "C" int32_t tmac_hip_rtn_params_dev(const void* W_dev, tmac_src_dtype_t src_dtype, int Mw, int K, int bits, int group_size, int zero_point,
                                           int scale_f16, float* scales_out_dev, float* zq_out_dev, int32_t* invalid_count_dev, void* stream) {
    const PackArg args[] = {{"W_dev", W_dev, true}, {"scales_out_dev", scales_out_dev, true}, {"zq_out_dev", zq_out_dev, true},
                            {"invalid_count_dev", invalid_count_dev, false}};
    RC_TRY(null_check(args));
    RC_TRY(src_dtype_check(src_dtype));
    if (bits < 1 || bits > 4) return fail(TMAC_HIP_E_ARG, "bits=%d: 1 to 4 are served", bits);
    if (Mw <= 0 || K <= 0 || group_size <= 0 || group_size % 4 || K % group_size)
        return fail(TMAC_HIP_E_ARG, "Mw=%d, K=%d and group_size=%d must be positive, group_size a multiple of 4 that divides K", Mw, K, group_size);
    RC_TRY(aligned_check(args));
    RC_TRY(ensure_device());
    RC_TRY(defer_barrier());
    hipStream_t st = (hipStream_t)stream;
    if (invalid_count_dev) HIP_TRY(hipMemsetAsync(invalid_count_dev, 0, sizeof(int32_t), st));
    return launched(launch_rtn_params(W_dev, src_dtype, Mw, K, bits, group_size, zero_point, scale_f16, scales_out_dev, zq_out_dev, nullptr,
                                      invalid_count_dev, st), "rtn_params");
}

extern "C" int32_t tmac_hip_ref_blob_bytes(int Mw, int K, int bits, const tmac_kcfg* cfg, tmac_dtype_t ref_float, size_t* a_bytes, size_t* s_bytes) {
    RC_TRY(float_dtype_check(ref_float, "ref_float"));
    Shape s;
    RC_TRY(make_shape(s, Mw, K, bits, cfg));
    if (a_bytes) *a_bytes = ref_weight_bytes(s);
    if (s_bytes) *s_bytes = ref_scale_elems(s) * dt_size((Dtype)ref_float);
    return TMAC_HIP_OK;
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

extern "C" int32_t tmac_hip_weights_kperm_id(const tmac_hip_weights* w, uint64_t* id) {
    if (!w || !id) return fail(TMAC_HIP_E_ARG, "null argument");
    *id = w->kperm ? w->kperm->h.id : 0;
    return TMAC_HIP_OK;
}
