// tmac_xform.h — the field rules of tmac_hip_xform (include/tmac_hip.h), said once for every path that takes a vector transform.
// Host code only; depends on include/tmac_hip.h and the C++ standard library (tests/cpp/xf_resolve_main.cc builds it with plain g++).
//
// xf_resolve turns the caller's struct into an XfSpec: kind and gate split, every field the kind does not read nulled.  Per kind
// (low byte of tmac_hip_xform::kind; the gate is bits 8..15, nothing above):
//
//   kind          gate       reads                                   must be NULL / 0                  ignored (nulled in the spec)
//   NONE (0)      refused    nothing                                 -                                 every field
//   NORM (1)      refused    residual, gamma, residual_out, keep*    -                                 in2
//   GLU (2)       0 / 1 / 2  in2 (required)                          -                                 residual, gamma, residual_out, keep
//   GLU_NORM (4)  0 / 1 / 2  in2, gamma (both required)              residual, residual_out, keep      -
//   3, 5 ...      -          "unknown transform kind", whatever the gate bits are
//   eps is copied as it comes for every kind.  (*) keep: see the sites.
//
// The three sites (XfSite) differ, and stay different, in this and nothing else:
//   XF_SITE_CHAIN (tmac_hip_chain_xform)   residual == TMAC_XF_CARRY is a tag (spec.carry, spec.residual null); keep is read by a NORM;
//                                          in2 is fp16; ALL FOUR pointers of the caller's struct must be 16-byte aligned, whatever the kind
//                                          reads (CARRY is no address).  Overlaps are the chain build's hazard analysis, not checked here.
//   XF_SITE_N1, XF_SITE_ROWS               CARRY is refused; keep is ignored by NORM and GLU (spec.keep = 0); in2 has the activations'
//   (tmac_hip_qgemm_fused_xf_dev;          dtype; only the pointers the kind reads are aligned.  xf_overlap_check: N1 -- every workgroup
//    .._xf_rows_dev, tmac_hip_debug_xf_rows)  reads B_dev, residual, gamma while one writes residual_out; ROWS -- the LUT builders read B_dev,
//                                          residual, gamma again after the row pass wrote residual_out, and the caller's in2 counts as read
//                                          even under a NORM, which ignores it.
//
// Order of the checks (the first fault names the refusal; all are TMAC_HIP_E_ARG): kind, gate, GLU_NORM's in2 / gamma / residual /
// residual_out / keep, GLU's in2, CARRY, alignment of in2 / residual / gamma / residual_out; then, where the entry point asks,
// xf_overlap_check: B_dev, residual, gamma, in2 (ROWS), then the outputs in order.  Around them, per entry point:
//   tmac_hip_qgemm_fused_xf_dev       xf_resolve; null arguments; B_dev, C_dev alignment; plan and route (TMAC_HIP_E_NOMATCH); xf_overlap_check
//   tmac_hip_qgemm_fused_xf_rows_dev  null arguments, C_dev alignment; xf_resolve; B_dev alignment; xf_overlap_check; then matrices, plan, route
//   tmac_hip_debug_xf_rows            its arguments; xf_resolve; B_dev, x_out_dev alignment; xf_overlap_check (the output is x_out_dev)
//   tmac_hip_chain_xform              xf_resolve alone (the call it belongs to is checked when it is recorded, overlaps when the chain is built)
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/tmac_hip.h"

namespace tmac_host {

int32_t fail(int32_t code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));   // tmac_runtime.cpp: sets the thread's message, returns code

// Alignment of caller-owned device pointers (include/tmac_hip.h, "Alignment"): every LUT build reads the activations 16 bytes at a time
// (uint4 / float4), every path reads its transform vectors and writes residual_out 16 bytes at a time.  A pointer below that is refused
// before anything is planned, queued or recorded.
constexpr size_t ACT_ALIGN = 16, XFORM_ALIGN = 16;
inline bool misaligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }
inline bool ranges_overlap(const void* a, size_t an, const void* b, size_t bn) {
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
    return a && b && pa < pb + bn && pb < pa + an;
}

enum XfSite { XF_SITE_N1, XF_SITE_ROWS, XF_SITE_CHAIN };

// a resolved transform: fields the kind does not read are null / 0 (the table above)
struct XfSpec {
    int kind = TMAC_XF_NONE;         // TMAC_XF_NONE / NORM / GLU / GLU_NORM
    int gate = 0;                    // GLU, GLU_NORM: 0 silu, 1 relu^2, 2 tanh-GELU (the kernels' XF_GATE_*)
    const void* in2 = nullptr;
    const float* residual = nullptr;
    bool carry = false;              // chain: the residual is the vector the latest kept NORM left in LDS
    const float* gamma = nullptr;
    float* residual_out = nullptr;
    float eps = 0.0f;
    int keep = 0;
};
inline bool xf_has_glu(const XfSpec& s) { return s.kind == TMAC_XF_GLU || s.kind == TMAC_XF_GLU_NORM; }   // reads a second vector
// Does an N > 1 call need k_xf_rows in front of the LUT build?  (residual_out and the rows' 1 / rms; GLU_NORM: always, gamma is required)
inline bool xf_needs_row_pass(const XfSpec& s) { return s.kind == TMAC_XF_GLU_NORM || (s.kind == TMAC_XF_NORM && (s.gamma || s.residual_out)); }

// Every field rule of the table.  TMAC_HIP_OK and *out, or fail(TMAC_HIP_E_ARG, ...) naming the field.  Allocates nothing, takes no lock,
// touches no global state.
int32_t xf_resolve(const tmac_hip_xform* xf, XfSite site, XfSpec* out);

// residual_out ([N][K] fp32) against what the call reads -- B_dev (act_esz bytes per value), residual, gamma, and at XF_SITE_ROWS the
// caller's in2 -- and against its outputs (named C_dev[i], or out_name).  TMAC_HIP_OK, or fail(TMAC_HIP_E_ARG, ...) naming the vector.
struct XfOut { const void* p; size_t bytes; };
int32_t xf_overlap_check(const XfSpec& s, XfSite site, const void* B_dev, size_t act_esz, const void* caller_in2, int K, int N, const XfOut* outs,
                         int nout, const char* out_name = nullptr);

}  // namespace tmac_host
