// tmac_quad_core.h — device functions shared by the QUAD-layout decode kernels: k_gemv_quad (tmac_quad.hip, one launch
// per fused GEMV group) and k_decode_chain (tmac_chain.hip, one persistent launch per recorded call sequence).
// The signed lookup follows tbl.cc:445-462 (see tmac_core.h); the LUT build is tmac_lut_build.h, the scalar and cross-lane helpers
// tmac_dev.h; here: the lookup and the vector transforms for N > 1 rows.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>

#include "tmac_core.h"
#include "tmac_dev.h"
#include "tmac_lut_build.h"

namespace tmac {

typedef uint32_t u32x4q __attribute__((ext_vector_type(4)));

typedef int qv4i_t __attribute__((ext_vector_type(4)));

// (x & m) | k in one VALU instruction (hipcc emits v_and_b32 + v_or_b32 for two literal operands: VOP3 takes no
// literals on gfx9, so the constants are kept in an SGPR and a VGPR)
__device__ __forceinline__ uint32_t q_and_or(uint32_t x, uint32_t m_sgpr, uint32_t k_vgpr) {
    uint32_t d;
    asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(d) : "v"(x), "s"(m_sgpr), "v"(k_vgpr));
    return d;
}

// Signed lookup for the MFMA accumulate: `all` = the four looked-up half-table entries, `neg` = those whose nibble has
// the negate bit, zero elsewhere.  The selector matrix weighs them +1 and -2: sum(all) - 2 sum(neg) = sum(pos) - sum(neg),
// exact in int32, and one v_perm_b32 less per four lookups than routing every entry to a plus or a minus word.
template <int H>
__device__ __forceinline__ void q_lookup4_pm(uint32_t w, uint32_t tab_lo, uint32_t tab_hi, uint32_t k3, uint32_t& all, uint32_t& neg) {
    const uint32_t x = H ? (w >> 4) : w;
    all = __builtin_amdgcn_perm(tab_hi, tab_lo, x & 0x07070707u);
    const uint32_t sel3 = q_and_or(x >> 1, 0x04040404u, k3);       // byte i: i (-> 0) or 4 + i (-> entry i) by the negate bit
    neg = __builtin_amdgcn_perm(all, 0u, sel3);
}

// ---- vector transforms for N > 1 activation rows (XA = XfRowsArgs, tmac_kernels.h) ----------------------------------------
// (row n, pair p) of an [N][K] operand: lut_ld8 behind element n * K
// NORM: t = fp32(in) + residual of (row n, pair p) -- the row pass (k_xf_rows) and every builder form it with this one fp32 rn add
template <class XA>
__device__ __forceinline__ void xf_rows_t8(const XA& a, const void* __restrict__ B, bool f16, int K, int n, int p, float (&t)[8]) {
    lut_ld8(B, f16, (size_t)n * K, p, t);
    if (a.residual != nullptr) {
        float u[8];
        lut_ld8(a.residual, false, (size_t)n * K, p, u);
#pragma unroll
        for (int i = 0; i < 8; ++i) t[i] = __fadd_rn(t[i], u[i]);
    }
}
// The gate of a GLU / GLU_NORM (bits 8..15 of tmac_hip_xform::kind, as the kernels carry it: 0 silu, 1 relu^2, 2 tanh-GELU), one
// expression per gate for all four places that apply one (k_gemv_quad, xf_rows_g8, k_decode_chain's reader form and its producer
// epilogue).  silu(v) * u = v / (1 + exp(-v)) * u: hardware exp2 and reciprocal (1 ulp each; specified to a tolerance).  GELU in its
// tanh form is the same expression with z = 2 * sqrt(2 / pi) * v * (1 + 0.044715 v^2) inside the exponential (0.5 (1 + tanh y) =
// sigmoid(2 y)): three more VALU.  relu^2 is exact arithmetic, specified to the bit: (max(v, 0) * max(v, 0)) * u, each product rounded.
constexpr int XF_GATE_SILU = 0, XF_GATE_RELU2 = 1, XF_GATE_GELU = 2;
__device__ __forceinline__ float xf_gate_silu(float v, float u) {
    return __fmul_rn(__fmul_rn(v, __builtin_amdgcn_rcpf(__fadd_rn(1.0f, __expf(-v)))), u);
}
__device__ __forceinline__ float xf_gate_relu2(float v, float u) {
    const float m = fmaxf(v, 0.0f);
    return __fmul_rn(__fmul_rn(m, m), u);
}
__device__ __forceinline__ float xf_gate_gelu(float v, float u) {
    const float z = __fmul_rn(v, __fmaf_rn(__fmul_rn(v, v), 1.5957691216f * 0.044715f, 1.5957691216f));
    return __fmul_rn(__fmul_rn(v, __builtin_amdgcn_rcpf(__fadd_rn(1.0f, __expf(-z)))), u);
}
// x[i] = gate(x[i]) * u[i].  `gate` is wave-uniform (a kernel argument or a descriptor field): one scalar branch around three straight
// loops, the silu loop being the code the kernels had before the selector existed.
template <int NE>
__device__ __forceinline__ void xf_gate_mul(int gate, float (&x)[NE], const float (&u)[NE]) {
    if (gate == XF_GATE_SILU) {
#pragma unroll
        for (int i = 0; i < NE; ++i) x[i] = xf_gate_silu(x[i], u[i]);
    } else if (gate == XF_GATE_RELU2) {
#pragma unroll
        for (int i = 0; i < NE; ++i) x[i] = xf_gate_relu2(x[i], u[i]);
    } else {
#pragma unroll
        for (int i = 0; i < NE; ++i) x[i] = xf_gate_gelu(x[i], u[i]);
    }
}
// the gate of an argument block: its `gate` field where it has one (XfRowsGateArgs), else silu -- a constant, and the code is the silu loop alone
template <class XA> __device__ __forceinline__ auto xf_rows_gate(const XA& a, int) -> decltype(a.gate) { return a.gate; }
template <class XA> __device__ __forceinline__ int xf_rows_gate(const XA&, long) { return XF_GATE_SILU; }
// GLU: g = gate(fp32(in)) * fp32(in2) of (row n, pair p), k_gemv_quad's expression with in2[n] in the activations' dtype -- the row pass of a
// GLU_NORM and every builder form it with this one function, so the builders recompute the g the row's sum was taken over, bit for bit
template <class XA>
__device__ __forceinline__ void xf_rows_g8(const XA& a, const void* __restrict__ B, bool f16, int K, int n, int p, float (&x)[8]) {
    float u[8];
    lut_ld8(B, f16, (size_t)n * K, p, x);
    lut_ld8(a.in2, f16, (size_t)n * K, p, u);
    xf_gate_mul(xf_rows_gate(a, 0), x, u);
}
// The transformed x[8] of (row n, pair p): what an XF instantiation of an N > 1 LUT builder (and the tap, k_xf_rows_tap) takes in place
// of its activation load.  NORM: (t * gamma) * r[n], k_gemv_quad's association (gamma first), r[n] from k_xf_rows; without gamma x = t
// untouched.  GLU: xf_rows_g8.  GLU_NORM (kind 4): (g * gamma) * r[n], r[n] from k_xf_rows' sum over g.  n is the row EVERY operand is read at: a builder
// that clamps padding rows passes the clamped row, so nothing is read beyond row N - 1.
template <class XA>
__device__ __forceinline__ void xf_rows_x8(const XA& a, const void* __restrict__ B, bool f16, int K, int n, int p, float (&x)[8]) {
    if (a.kind == 1) {
        xf_rows_t8(a, B, f16, K, n, p, x);
        if (a.gamma != nullptr) {
            float g[8];
            lut_ld8(a.gamma, false, 0, p, g);
            const float r = a.r[n];
#pragma unroll
            for (int i = 0; i < 8; ++i) x[i] = __fmul_rn(__fmul_rn(x[i], g[i]), r);
        }
    } else {
        xf_rows_g8(a, B, f16, K, n, p, x);
        if (a.kind == 4) {
            float g[8];
            lut_ld8(a.gamma, false, 0, p, g);
            const float r = a.r[n];
#pragma unroll
            for (int i = 0; i < 8; ++i) x[i] = __fmul_rn(__fmul_rn(x[i], g[i]), r);
        }
    }
}
template <class XA> __device__ __forceinline__ const XA& xf_rows_arg(const XA& a) { return a; }

// ---- the gather of an act-order permutation for N > 1 rows ------------------------------------------------------------------------
// The same slot of the builders -- "x[8] of (row n, pair p) in place of the activation load" -- filled with x[n][perm[8 p .. 8 p + 7]]: two
// 16-byte index loads, then eight element loads.  Every index is < K (tmac_hip_kperm_from_gidx_dev refuses anything else), so the element
// loads stay inside row n, which the builder has clamped already.
struct GatherRowsArgs {
    const int32_t* perm;     // int32 [K], 16-byte aligned
};
__device__ __forceinline__ void xf_rows_x8(const GatherRowsArgs& a, const void* __restrict__ B, bool f16, int K, int n, int p, float (&x)[8]) {
    const int4* ip = reinterpret_cast<const int4*>(a.perm) + 2 * (size_t)p;
    const int4 i0 = ip[0], i1 = ip[1];
    const int k8[8] = {i0.x, i0.y, i0.z, i0.w, i1.x, i1.y, i1.z, i1.w};
    if (f16) {
        const __half* xb = reinterpret_cast<const __half*>(B) + (size_t)n * K;
#pragma unroll
        for (int i = 0; i < 8; ++i) x[i] = __half2float(xb[k8[i]]);
    } else {
        const float* xb = reinterpret_cast<const float*>(B) + (size_t)n * K;
#pragma unroll
        for (int i = 0; i < 8; ++i) x[i] = xb[k8[i]];
    }
}

}  // namespace tmac
