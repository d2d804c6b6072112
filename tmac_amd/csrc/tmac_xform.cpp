// tmac_xform.cpp — the field rules of tmac_hip_xform: the table and the order of the checks are in tmac_xform.h.
#include "tmac_xform.h"

using namespace tmac_host;

// tmac_hip_xform::kind split into the kind (low byte) and the gate of a GLU / GLU_NORM (bits 8..15: TMAC_XF_GATE_*)
static int32_t split_kind(int32_t kind, XfSpec* s) {
    const int k = kind & 0xff, g = kind & ~0xff;
    if (k != TMAC_XF_NONE && k != TMAC_XF_NORM && k != TMAC_XF_GLU && k != TMAC_XF_GLU_NORM) return fail(TMAC_HIP_E_ARG, "unknown transform kind %d", kind);
    if (g != 0 && (k == TMAC_XF_NONE || k == TMAC_XF_NORM))
        return fail(TMAC_HIP_E_ARG, "transform kind %d takes no gate: bits 8..15 of kind (0x%x here) select the gate of a GLU or GLU_NORM", k, (unsigned)g);
    if (g != TMAC_XF_GATE_SILU && g != TMAC_XF_GATE_RELU2 && g != TMAC_XF_GATE_GELU)
        return fail(TMAC_HIP_E_ARG, "unknown gate 0x%x in transform kind 0x%x (TMAC_XF_GATE_SILU, _RELU2 or _GELU in bits 8..15, nothing above)", (unsigned)g, (unsigned)kind);
    s->kind = k; s->gate = g >> 8;
    return TMAC_HIP_OK;
}

int32_t tmac_host::xf_resolve(const tmac_hip_xform* xf, XfSite site, XfSpec* out) {
    XfSpec s;
    const int32_t krc = split_kind(xf->kind, &s);
    if (krc) return krc;
    const bool chain = site == XF_SITE_CHAIN, norm = s.kind == TMAC_XF_NORM, glu_norm = s.kind == TMAC_XF_GLU_NORM;
    if (glu_norm) {
        if (!xf->in2) return fail(TMAC_HIP_E_ARG, "GLU_NORM needs a second vector (in2)");
        if (!xf->gamma) return fail(TMAC_HIP_E_ARG, "GLU_NORM needs the norm weights (gamma)");
        if (xf->residual) return fail(TMAC_HIP_E_ARG, "GLU_NORM takes no residual: the field must be NULL");
        if (xf->residual_out) return fail(TMAC_HIP_E_ARG, "GLU_NORM writes no residual_out: the field must be NULL");
        if (xf->keep) return fail(TMAC_HIP_E_ARG, "GLU_NORM keeps no vector: keep must be 0");
    }
    if (s.kind == TMAC_XF_GLU && !xf->in2) return fail(TMAC_HIP_E_ARG, "GLU needs a second vector");
    s.carry = xf->residual == TMAC_XF_CARRY;
    if (norm && s.carry && !chain)
        return fail(TMAC_HIP_E_ARG, "TMAC_XF_CARRY names a vector kept inside a chain launch: outside a recording the residual is a vector in memory");
    s.eps = xf->eps;
    if (xf_has_glu(s)) s.in2 = xf->in2;
    if (norm) {
        s.residual = s.carry ? nullptr : xf->residual;
        s.residual_out = xf->residual_out;
        s.keep = chain ? xf->keep : 0;
    }
    s.carry = s.carry && norm;
    if (norm || glu_norm) s.gamma = xf->gamma;
    // the chain aligns the caller's four pointers whatever the kind reads, the other sites those of the spec (CARRY is no address)
    const struct { const void* caller; const void* read; const char* name; } vec[] = {
        {xf->in2, s.in2, "in2"}, {xf->residual == TMAC_XF_CARRY ? nullptr : xf->residual, s.residual, "residual"},
        {xf->gamma, s.gamma, "gamma"}, {xf->residual_out, s.residual_out, "residual_out"}};
    for (const auto& v : vec)
        if (misaligned(chain ? v.caller : v.read, XFORM_ALIGN))
            return fail(TMAC_HIP_E_ARG, "transform vector %s must be %zu-byte aligned (read or written 16 bytes at a time)", v.name, XFORM_ALIGN);
    *out = s;
    return TMAC_HIP_OK;
}

int32_t tmac_host::xf_overlap_check(const XfSpec& s, XfSite site, const void* B_dev, size_t act_esz, const void* caller_in2, int K, int N,
                                    const XfOut* outs, int nout, const char* out_name) {
    if (!s.residual_out) return TMAC_HIP_OK;
    const bool rows = site == XF_SITE_ROWS;
    const size_t NK = (size_t)N * K;
    const struct { const void* p; size_t n; const char* name; } rd[] = {{B_dev, NK * act_esz, "B_dev"}, {s.residual, NK * 4, "residual"}, {s.gamma, (size_t)K * 4, "gamma"},
                                                                       {rows ? caller_in2 : nullptr, NK * act_esz, "in2"}};
    for (const auto& r : rd)
        if (ranges_overlap(s.residual_out, NK * 4, r.p, r.n))
            return fail(TMAC_HIP_E_ARG, "residual_out overlaps %s, which %s (alternate between two buffers)", r.name,
                        rows ? "the LUT build reads after the row pass has written it" : "every workgroup reads while one writes");
    for (int i = 0; i < nout; ++i)
        if (ranges_overlap(s.residual_out, NK * 4, outs[i].p, outs[i].bytes))
            return out_name ? fail(TMAC_HIP_E_ARG, "residual_out overlaps %s", out_name) : fail(TMAC_HIP_E_ARG, "residual_out overlaps C_dev[%d]", i);
    return TMAC_HIP_OK;
}
