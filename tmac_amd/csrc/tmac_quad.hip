// tmac_quad.hip — k_gemv_quad: fused LUT build + GEMV (N = 1 decode), a wave owns a row quad.  Production path.
//
// Reference semantics: lut_ctor.cc:38-266 (LUT build, bit-exact), tbl.cc:435-529 / 586-628 (lookup, exact integer sums,
// per-act-group fp32 scale-apply), qgemm.py:170-174,192-206 (bit-plane combine, scale-final).  Work decomposition:
// a WAVE owns a row quad (4 output rows): its 64 lanes hold 64 consecutive 8-table units (QUAD layout,
// tmac_layout.h), so every weight instruction reads 1 KiB contiguous, the LUT in LDS is read conflict-free (lane u
// reads 16 B at u*16), and the reduction over K is wave-local (DPP within rows of 16 lanes + 2 cross-row moves).
//   WPQ = 1     : one wave does all of K for its quad                       (many quads: q/k/v, gate/up)
//   WPQ = 2,3,4 : that many waves split the K steps of a quad, combined in LDS  (few quads: o, down)
// Workgroups (512 / 768 / 1024 threads) are persistent, build the LUT once while their first weight fragments are in
// flight, then walk their (quad, step) list.  Template parameters: BITS 2|4; ZP zero points; SM 0 per-group scales /
// 2 unified scale applied last (BitNet); LUTSRC 1 build the LUT in-kernel / 0 copy the image k_preprocess wrote;
// NR tables built per thread; FT threads; WPQ waves per quad; DUMP integer tap; ACC 1 v_mfma_i32_16x16x64_i8
// accumulate / 0 v_mqsad_pk_u16_u8 (A/B variant); XF a vector transform of the activations (residual add + RMSNorm,
// gate(in) * in2, the gate silu, relu^2 or tanh-GELU: tmac_hip_qgemm_fused_xf_dev) between the activation loads and the table build, where every workgroup
// holds the whole vector; BI the bias of a handle added in front of the output's store (y = W x + b).  DESIGN.md 4.1, 4.2, 4.6, 4.15.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>
#include <type_traits>

#include "tmac_core.h"
#include "tmac_kernels.h"
#include "tmac_fastdiv.h"
#include "tmac_quad_core.h"
#include "tmac_select.h"

namespace tmac {


// weights of (local quad lq, step st) + the lane's scales (rows beta0, beta0+1 of its unit's scale group)
template <int BITS, bool ZP, int SM, int ACC, bool SCF16>
__device__ __forceinline__ void load_q(WFrag<BITS>& f, const FusedArgs& a, const FusedMat& M, int lq, int st, int nst, int lane) {
    constexpr int NJ = 8 * BITS / 8;
    constexpr int per = ZP ? 2 : 1;
    const int u = st * 64 + lane;
    // Scale words go through scalar locals and are stored to f.sraw with constant subscripts at the end: stores to
    // different elements in the two dtype branches get sunk into one store with a run-time subscript, which
    // keeps the whole fragment in scratch memory.
    uint32_t r0 = 0, r1 = 0, r2 = 0, r3 = 0;
    if (SM == 0 && ACC == 1) {
        // epilogue role of this lane: row beta = lane & 3, units st*64 + 16g + 4*lg .. +3 (g = (lane & 15) >> 2, lg = lane >> 4)
        // sraw[2*gi], sraw[2*gi+1]: scale (, zero) of act-group pair gi; f16 packs both into sraw[2*gi]
        // Loads are unconditional with clamped indices (no exec-mask branches around them); units past K read zero
        // tables from LDS, so what the clamped lanes load never reaches a result.
        // scale group of unit st*64 + c: st * (64 >> gs_shift) + (c >> gs_shift)  (a scale group never straddles a
        // step: gs <= 2048); the lane part is loop-invariant, the step part scalar, the address a uniform base plus a
        // 32-bit lane offset
        const int c0 = 4 * (lane & 12) + 4 * (lane >> 4);
        const uint32_t sg_step = (uint32_t)st * (64u >> a.gs_shift);
        const uint32_t row0 = (uint32_t)lq * (uint32_t)a.nsg;
        const char* scb = reinterpret_cast<const char*>(M.SC);
#pragma unroll
        for (int gi = 0; gi < 2; ++gi) {
            uint32_t v0 = 0, v1 = 0;
            if (gi == 0 || a.gs_shift < 2) {      // gs >= 128: both act-group pairs of the lane share the scale group (the epilogue reads pair 0)
                const uint32_t sg = min(sg_step + (uint32_t)((c0 + 2 * gi) >> a.gs_shift), (uint32_t)a.nsg - 1u);
                const uint32_t sidx = ((row0 + sg) * 4 + (lane & 3)) * per;
                if (SCF16) {
                    const char* ph = scb + (size_t)(sidx * 2u);
                    if (ZP) v0 = *reinterpret_cast<const uint32_t*>(ph);
                    else v0 = *reinterpret_cast<const unsigned short*>(ph);
                } else {
                    const uint32_t* p32 = reinterpret_cast<const uint32_t*>(scb + (size_t)(sidx * 4u));
                    v0 = p32[0];
                    if (ZP) v1 = p32[1];
                }
            }
            if (gi == 0) { r0 = v0; r1 = v1; } else { r2 = v0; r3 = v1; }
        }
    }
    if (ACC == 1 || u < a.nu) {   // nst*64 lanes of every step exist in the QUAD layout (zero padded)
        const uint4* wp = M.W + (size_t)((uint32_t)(lq * nst + st) * (uint32_t)(NJ * 64)) + lane;   // uniform base + lane
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const u32x4q v = __builtin_nontemporal_load(reinterpret_cast<const u32x4q*>(wp + (size_t)j * 64));
            f.wd[4 * j] = v.x; f.wd[4 * j + 1] = v.y; f.wd[4 * j + 2] = v.z; f.wd[4 * j + 3] = v.w;
        }
        if (SM == 0 && ACC == 0) {
            // rows beta0, beta0+1 of this unit's scale group: fp32 -> one word per element, f16 -> two per word
            const int sg = u >> a.gs_shift;
            const uint32_t sidx = (((uint32_t)lq * (uint32_t)a.nsg + (uint32_t)sg) * 4 + 2 * (lane & 1)) * per;
            if (SCF16) {
                const uint32_t* p32 = reinterpret_cast<const uint32_t*>(reinterpret_cast<const __half*>(M.SC) + sidx);
                r0 = p32[0];
                if (ZP) r1 = p32[1];
            } else {
                const uint32_t* p32 = reinterpret_cast<const uint32_t*>(M.SC) + sidx;
                r0 = p32[0]; r1 = p32[1];
                if (ZP) { r2 = p32[2]; r3 = p32[3]; }
            }
        }
    }
    if (SM == 0) { f.sraw[0] = r0; f.sraw[1] = r1; f.sraw[2] = r2; f.sraw[3] = r3; }
}


// ACC 0: v_mqsad_pk_u16_u8 accumulate (VALU).  ACC 1: v_mfma_i32_16x16x64_i8 accumulate (matrix pipe), see
// k_gemv_fused for the operand construction; with 64 lanes = 64 units of one quad, source lane l = 16g + i and
// D[i][4g+beta] lands in lane l' = 16*(i/4) + 4g + beta, register i%4: lane l' owns output row beta and the four
// units 16g + 4*(l'/16) .. +3 of the step (two act groups, one 128-wide scale group).
// XF (LUTSRC 1, ACC 1, no tap, one activation row): the argument block carries the transform's operands (FusedXfArgs); every line of it
// sits under if constexpr (XF).  GN (with XF): the instantiation serves TMAC_XF_GLU_NORM (xf_kind 4) and nothing else -- kinds 1 and 2 keep
// the code they had (measured: sharing one instantiation moved the GLU by 1 %, profiles/r13_glunorm_bench.txt).
// GT (with XF): the gate of the GLU / GLU_NORM is a run-time choice (a.xf_kind >> 8) -- instantiations of their own for relu^2 and GELU.  Inside
// the GN ones the selector cost the six-tables-per-thread forms (K > 4096 at 512 threads) up to 4 VGPRs; inside the shared NORM / GLU ones it
// cost no register, but the silu GLU of llama-2-7B's down 0.14 us in 8.2, outside the spread of the parent's runs
// (profiles/r14_gate_resources.txt, profiles/r14_gate_bench.txt).  Without GT the gate is silu, spelled out: the code of before.
// GA (LUTSRC 1, ACC 1, no tap, no transform): the gather of an act-order matrix -- the lane's eight activations are x[perm[8 p .. 8 p + 7]]
// instead of x[8 p .. 8 p + 7] (FusedPermArgs); every line of it sits under if constexpr (GA), and everything from the act-group scale on is
// the text of the plain build.
// BI (MFMA form, per-group scales, no tap; with XF: NORM and the silu GLU): y = W x + b -- the matrix' bias (FusedBiasArgs / FusedXfBiasArgs:
// the handle's fp32 copy, padded to whole quads, or null) is added to the output value in front of its one store, one correctly rounded
// add; every line of it sits under if constexpr (BI).  Lane l < 4 loads the bias of its own output row at the store (one vector load of 4
// bytes per output).  The other candidate -- the quad's four biases from their ONE wave-uniform address through the scalar unit's load path,
// which does not queue behind the weight fragments in flight as a vector load does -- measured 1.7 % SLOWER over the eight llama-2-7B
// N = 1 cells (seven of eight; profiles/r25_bias.txt), so it is not in the code.
template <int BITS, bool ZP, int SM, int LUTSRC, int NR, int FT, int WPQ, bool DUMP, int ACC, bool SCF16, bool EARLY, bool XF = false, bool GN = false, bool GT = false,
          bool GA = false, bool BI = false>
__global__ __launch_bounds__(FT) void k_gemv_quad(std::conditional_t<BI, std::conditional_t<XF, FusedXfBiasArgs, FusedBiasArgs>,
                                                                     std::conditional_t<XF, FusedXfArgs, std::conditional_t<GA, FusedPermArgs, FusedArgs>>> a) {
    static_assert(!XF || (LUTSRC == 1 && ACC == 1 && !DUMP), "the transform lives in the in-kernel LUT build of the MFMA form");
    static_assert(!GA || (LUTSRC == 1 && ACC == 1 && !DUMP && !XF && SM == 0), "the gather lives in the in-kernel LUT build of the MFMA form, per-group scales");
    static_assert(!GN || XF, "GLU_NORM is a transform");
    static_assert(!GT || XF, "the gate belongs to a transform");
    static_assert(!BI || (ACC == 1 && SM == 0 && !DUMP && !GA && !GN && !GT), "the bias: MFMA form, per-group scales, no tap; NORM and the silu GLU");
    extern __shared__ uint4 lds[];
    const unsigned long long t_entry = DUMP ? __builtin_amdgcn_s_memtime() : 0ull;   // before the first kernel-argument load
    constexpr int NWV = FT / 64, IPI = NWV / WPQ;
    const Shape& s = a.s;
    // the wave index is uniform but the compiler cannot prove it from threadIdx: readfirstlane moves every
    // per-wave quantity (quad, step, base pointers, loop control) to SGPRs / the scalar ALU
    const int tid = threadIdx.x, w = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int n = blockIdx.y;
    const int T = s.K / 4, nu = a.nu, G = a.G, nst = (nu + 63) >> 6;
    const int tstride = nst * 64 + 1;                            // whole steps: units past K hold zero tables
    uint4* tab = lds;                                            // [4][tstride]
    const int GP = nst * 32;                                     // act groups of the padded steps (>= G)
    // MFMA accumulate with per-group scales: the epilogue works on the plane-combined integer (see compute_mfma), which
    // wants ls / 2 and lb / 2 -- stored halved (exact) instead of being halved per use
    constexpr bool HALVES = (ACC == 1 && SM != 2);
    constexpr float LSK = HALVES ? 0.5f : 1.0f;
    float* l_ls = reinterpret_cast<float*>(lds + 4 * tstride);   // [GP]  (groups past K: 0)
    float* l_lb = l_ls + GP;                                     // [GP]
    float* l_red = l_lb + GP;                                    // [2][NWV][4][4] partials (WPQ == 2 / SM 2)
    float* l_scr = l_red + 2 * NWV * 16;                         // SM 2 build scratch: [NWV] maxima + [T/8] chunk sums
    // Per-matrix fields: a cursor (one for the prefetch, one for the consumption) caches the current matrix' pointers
    // and quad range in SGPRs and advances when a quad index leaves the range (quads only grow).  Looking the matrix
    // up per step — run-time indexing of a.m[], or select chains over four copies — costs tens of scalar
    // instructions per step, and the scalar pipe issues no faster than the vector pipe.
    const int nmat = a.nmat;
    const int total_q = a.m[nmat - 1].nb_end;                    // cumulative QUAD counts
    struct MatCur { FusedMat m; int base, mi, end; };          // end: first quad past this matrix (INT_MAX for the last)
    auto seek = [&](MatCur& c, int gq) {
        while (gq >= c.end) { c.base = c.m.nb_end; ++c.mi; c.m = a.m[c.mi]; c.end = (c.mi + 1 < nmat) ? c.m.nb_end : 0x7fffffff; }
    };
    MatCur pc = {a.m[0], 0, 0, nmat > 1 ? a.m[0].nb_end : 0x7fffffff}, cc = pc;

#define QSTAMP(i) do { if (DUMP && a.stamps && lane == 0 && (w == 0 || w == NWV - 1)) a.stamps[((size_t)blockIdx.x * 2 + (w ? 1 : 0)) * 8 + (i)] = __builtin_amdgcn_s_memtime(); } while (0)
    QSTAMP(0);
    if (DUMP && a.stamps && lane == 0 && (w == 0 || w == NWV - 1)) a.stamps[((size_t)blockIdx.x * 2 + (w ? 1 : 0)) * 8 + 7] = t_entry;

    // ---- 1. activation loads for the LUT build (issued first: vmcnt retires in order) ----------
    // A lane builds the two consecutive tables 2p, 2p+1 (8 activations, one 16-byte fp16 load) of pair p = r*FT + tid:
    // one uint4 LDS store, and the act-group scale (abs-max over 8 lanes, two exact divisions) is computed once per two
    // tables.
    constexpr int NP = NR / 2;                                   // pairs per thread
    const int P = T / 2;
    uint32_t xr[NP][8];
    if constexpr (GA) {
        // Two dependent loads: the pair's eight source indices (two 16-byte loads, clamped like the plain pair), then eight elements.  Every
        // index is < K (tmac_hip_kperm_from_gidx_dev refuses anything else), so the element loads stay inside row n.  xr holds fp32, the
        // form the XF instantiations use.  Issued here, in front of the weight fragments: vmcnt retires in order.
#pragma unroll
        for (int r = 0; r < NP; ++r) {
            const int p = min(r * FT + tid, P - 1);
            const int4* ip = reinterpret_cast<const int4*>(a.perm) + 2 * (size_t)p;
            const int4 i0 = ip[0], i1 = ip[1];
            const int k8[8] = {i0.x, i0.y, i0.z, i0.w, i1.x, i1.y, i1.z, i1.w};
            if (a.act_f16) {
                const __half* xb = reinterpret_cast<const __half*>(a.B) + (size_t)n * s.K;
#pragma unroll
                for (int i = 0; i < 8; ++i) xr[r][i] = __float_as_uint(__half2float(xb[k8[i]]));
            } else {
                const uint32_t* xb = reinterpret_cast<const uint32_t*>(a.B) + (size_t)n * s.K;
#pragma unroll
                for (int i = 0; i < 8; ++i) xr[r][i] = xb[k8[i]];
            }
        }
    }
    if (LUTSRC == 1 && !GA) {
#pragma unroll
        for (int r = 0; r < NP; ++r) {
            const int p = min(r * FT + tid, P - 1);     // clamped, not predicated (see load_q)
            if (a.act_f16) {
                const uint4 v = reinterpret_cast<const uint4*>(reinterpret_cast<const __half*>(a.B) + (size_t)n * s.K)[p];
                xr[r][0] = v.x; xr[r][1] = v.y; xr[r][2] = v.z; xr[r][3] = v.w;
            } else {
                const uint4* src = reinterpret_cast<const uint4*>(reinterpret_cast<const float*>(a.B) + (size_t)n * s.K) + 2 * (size_t)p;
                const uint4 v0 = src[0], v1 = src[1];
                xr[r][0] = v0.x; xr[r][1] = v0.y; xr[r][2] = v0.z; xr[r][3] = v0.w;
                xr[r][4] = v1.x; xr[r][5] = v1.y; xr[r][6] = v1.z; xr[r][7] = v1.w;
            }
        }
    }
    // XF: the transform's operands for the lane's own pairs, clamped like xr: NORM residual (xa) and gamma (xg), GLU in2 (xa), GLU_NORM
    // (xf_kind 4) in2 (xa) and gamma (xg)
    uint32_t xa[XF ? NP : 1][8], xg[XF ? NP : 1][8];
    if constexpr (XF) {
#pragma unroll
        for (int r = 0; r < NP; ++r) {
            const int p = min(r * FT + tid, P - 1);
#pragma unroll
            for (int i = 0; i < 8; ++i) { xa[r][i] = 0u; xg[r][i] = 0u; }
            const void* src_a = (!GN && a.xf_kind == 1) ? (const void*)a.residual : a.in2;
            if (src_a != nullptr) {
                if ((GN || (GT ? a.xf_kind != 1 : a.xf_kind == 2)) && a.act_f16) {      // (GT: a GLU's xf_kind carries its gate)
                    const uint4 v = reinterpret_cast<const uint4*>(src_a)[p];
                    xa[r][0] = v.x; xa[r][1] = v.y; xa[r][2] = v.z; xa[r][3] = v.w;
                } else {
                    const uint4* src = reinterpret_cast<const uint4*>(src_a) + 2 * (size_t)p;
                    const uint4 v0 = src[0], v1 = src[1];
                    xa[r][0] = v0.x; xa[r][1] = v0.y; xa[r][2] = v0.z; xa[r][3] = v0.w;
                    xa[r][4] = v1.x; xa[r][5] = v1.y; xa[r][6] = v1.z; xa[r][7] = v1.w;
                }
            }
            if ((GN || a.xf_kind == 1) && a.gamma != nullptr) {
                const uint4* src = reinterpret_cast<const uint4*>(a.gamma) + 2 * (size_t)p;
                const uint4 v0 = src[0], v1 = src[1];
                xg[r][0] = v0.x; xg[r][1] = v0.y; xg[r][2] = v0.z; xg[r][3] = v0.w;
                xg[r][4] = v1.x; xg[r][5] = v1.y; xg[r][6] = v1.z; xg[r][7] = v1.w;
            }
        }
    }
    float xrs = 1.0f;                 // XF, NORM with gamma / GLU_NORM: 1 / rms, known behind the cross-wave sum below
    bool xnorm = false;
    auto unpack = [&](int r, float (&x)[8]) {
        if (!XF && !GA && a.act_f16) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const __half2 hh = *reinterpret_cast<const __half2*>(&xr[r][i]);
                x[2 * i] = __low2float(hh); x[2 * i + 1] = __high2float(hh);
            }
        } else {      // (XF: xr holds the transformed vector as fp32; GA: the gathered one)
#pragma unroll
            for (int i = 0; i < 8; ++i) x[i] = __uint_as_float(xr[r][i]);
        }
        if constexpr (XF) {
            if (xnorm) {
#pragma unroll
                for (int i = 0; i < 8; ++i) x[i] = __fmul_rn(x[i], xrs);
            }
        }
    };
    // ---- 1b. XF: the element-wise part of the transform, in place in xr (fp32 from here on) -----
    // Before the weight fragments are issued: it waits for the operand loads, and nothing else is in flight yet.  NORM: t = in +
    // residual (fp32 rn), t to residual_out by the ONE workgroup that owns the pair (p mod gridDim.x: a grid of one owns them all),
    // the lane's part of sum t^2, and t * gamma; 1 / rms multiplies in unpack, once the sum is known.  Without gamma x = t, untouched:
    // the table build then sees the bits a plain call on t would.  GLU: x = gate(in) * in2 (silu, GELU: the hardware exp and reciprocal)
    // (tmac_chain.hip's formula).  The transformed vector stays in the registers the raw one arrived in (xr is [NP][8] for fp32
    // activations anyway); the operands are dead behind this block.  GLU_NORM: g = the GLU's x, then the NORM's tail on g -- the lane's
    // part of sum g^2 (own pairs only: a clamped lane holds a copy of the last pair), g * gamma, 1 / rms in unpack.
    float xss = 0.f;
    if constexpr (XF) {
        const bool in_f16 = a.act_f16 != 0;
#pragma unroll
        for (int r = 0; r < NP; ++r) {
            const int p = r * FT + tid;
            float x[8];
            if (in_f16) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const __half2 hh = *reinterpret_cast<const __half2*>(&xr[r][i]);
                    x[2 * i] = __low2float(hh); x[2 * i + 1] = __high2float(hh);
                }
            } else {
#pragma unroll
                for (int i = 0; i < 8; ++i) x[i] = __uint_as_float(xr[r][i]);
            }
            if (!GN && a.xf_kind == 1) {
                if (a.residual != nullptr) {
#pragma unroll
                    for (int i = 0; i < 8; ++i) x[i] = __fadd_rn(x[i], __uint_as_float(xa[r][i]));
                }
                if (p < P) {
                    if (a.residual_out != nullptr && (uint32_t)p % gridDim.x == blockIdx.x) {
                        float4* ro = reinterpret_cast<float4*>(a.residual_out) + 2 * (size_t)p;
                        ro[0] = make_float4(x[0], x[1], x[2], x[3]);
                        ro[1] = make_float4(x[4], x[5], x[6], x[7]);
                    }
#pragma unroll
                    for (int i = 0; i < 8; ++i) xss = __fmaf_rn(x[i], x[i], xss);
                }
                if (a.gamma != nullptr) {
#pragma unroll
                    for (int i = 0; i < 8; ++i) x[i] = __fmul_rn(x[i], __uint_as_float(xg[r][i]));
                }
            } else {
                float u[8];
                if (in_f16) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const __half2 hh = *reinterpret_cast<const __half2*>(&xa[r][i]);
                        u[2 * i] = __low2float(hh); u[2 * i + 1] = __high2float(hh);
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < 8; ++i) u[i] = __uint_as_float(xa[r][i]);
                }
                // x = gate(x) * u, the gate by a.xf_kind >> 8 (uniform): silu, relu^2 or tanh-GELU (tmac_quad_core.h)
                if constexpr (!GT) {      // silu, spelled out: the loop these instantiations had before the selector existed
#pragma unroll
                    for (int i = 0; i < 8; ++i)
                        x[i] = __fmul_rn(__fmul_rn(x[i], __builtin_amdgcn_rcpf(__fadd_rn(1.0f, __expf(-x[i])))), u[i]);
                } else {
                    xf_gate_mul(a.xf_kind >> 8, x, u);
                }
                if constexpr (GN) {
                    if (p < P) {
#pragma unroll
                        for (int i = 0; i < 8; ++i) xss = __fmaf_rn(x[i], x[i], xss);
                    }
#pragma unroll
                    for (int i = 0; i < 8; ++i) x[i] = __fmul_rn(x[i], __uint_as_float(xg[r][i]));
                }
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) xr[r][i] = __float_as_uint(x[i]);
        }
    }

    // ---- 2. this wave's work: quads slot, slot + stride, ...; steps h, h + WPQ, ... of each ------
    const int slot0 = blockIdx.x * IPI + w / WPQ, h = w % WPQ, stride = gridDim.x * IPI;
    constexpr int RING = (BITS <= 2) ? 4 : 2;      // weight fragments in flight per wave (register budget)
    WFrag<BITS> f0, f1, f2, f3;
    int p_q = (h < nst) ? slot0 : total_q, p_st = h;    // prefetch cursor (a wave without steps, WPQ > nst, never issues)
    auto issue = [&](WFrag<BITS>& f) {
        if (p_q < total_q) {
            seek(pc, p_q);
            load_q<BITS, ZP, SM, ACC, SCF16>(f, a, pc.m, p_q - pc.base, p_st, nst, lane);
            p_st += WPQ;
            if (p_st >= nst) { p_st = h; p_q += stride; }
        }
    };
    // When the weight loads are issued matters more than anything else in this kernel (measured, profiles/r01_tune_quad.txt):
    // issued first, as a prefetch, they occupy the CU's 64 B/clk load path for 1-2 us while the VALU idles, and the LUT
    // build cannot start before the wave's own loads have all returned (its s_waitcnt is vmcnt(0): loads sit under
    // wave-dependent branches).  So: wait for the activation registers alone (the empty asm reads them, the compiler
    // puts its s_waitcnt in front), THEN issue the fragments — the LUT build below is pure VALU and overlaps the weight
    // stream — or, with two workgroups per CU competing for the load path, after the LUT build.
    constexpr bool early = LUTSRC == 1 && EARLY;      // chosen by the launcher: at most one workgroup per CU
    if (LUTSRC == 1) {
#pragma unroll
        for (int r = 0; r < NP; ++r)
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (i < 4 || XF || GA || !a.act_f16) asm volatile("" :: "v"(xr[r][i]));
    }
    if (early) {
        issue(f0); issue(f1);
        if (RING == 4) { issue(f2); issue(f3); }
    }
    QSTAMP(1);
    if constexpr (XF) {
        // NORM with gamma, GLU_NORM: the mean square.  A wave sum per wave (four DPP steps inside the rows of 16 lanes, the four row sums through
        // readlane), the partials through LDS (l_red: idle until the first finish_quad, behind the barrier that ends section 3), added in
        // wave order by every thread.  The barrier is LDS-only: __syncthreads() carries s_waitcnt vmcnt(0) and would wait for the weight
        // fragments issued a moment ago.
        if ((GN || a.xf_kind == 1) && a.gamma != nullptr) {
            float ss = xss;
            ss = __fadd_rn(ss, dpp_f<0xB1>(ss)); ss = __fadd_rn(ss, dpp_f<0x4E>(ss));
            ss = __fadd_rn(ss, dpp_f<0x141>(ss)); ss = __fadd_rn(ss, dpp_f<0x140>(ss));     // row_half_mirror, row_mirror
            const int ssb = __builtin_bit_cast(int, ss);
            const float sw = __fadd_rn(__fadd_rn(__builtin_bit_cast(float, __builtin_amdgcn_readlane(ssb, 0)), __builtin_bit_cast(float, __builtin_amdgcn_readlane(ssb, 16))),
                                       __fadd_rn(__builtin_bit_cast(float, __builtin_amdgcn_readlane(ssb, 32)), __builtin_bit_cast(float, __builtin_amdgcn_readlane(ssb, 48))));
            if (lane == 0) l_red[w] = sw;
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            float tot = 0.f;
#pragma unroll
            for (int ww = 0; ww < NWV; ++ww) tot = __fadd_rn(tot, l_red[ww]);
            xrs = __builtin_amdgcn_rsqf(__fmaf_rn(tot, __builtin_amdgcn_rcpf((float)s.K), a.eps));
            xnorm = true;
        }
    }

    // ---- 3. LUT into LDS (all FT threads) ------------------------------------------------------
    // The constructor of tmac_lut_build.h.  In this kernel's own words stay the fp16 unpack, pass 1 of the unified-scale path with its two
    // divisions and the act-group scale: through the shared pieces some instantiations changed schedule or register counts
    // (profiles/r18_lut_build_refactor.txt).
    if (LUTSRC == 0) {
        const uint4* src = reinterpret_cast<const uint4*>(a.qlut_lds) + (size_t)n * 4 * a.tstride;   // image stride (k_preprocess)
#pragma unroll
        for (int j4 = 0; j4 < 4; ++j4)
            for (int u = tid; u < nu; u += FT) {
                uint4 v = src[j4 * a.tstride + u];
                if (ACC == 1) { v.x ^= 0x80808080u; v.y ^= 0x80808080u; v.z ^= 0x80808080u; v.w ^= 0x80808080u; }
                tab[j4 * tstride + u] = v;
            }
        if (SM == 2) { if (tid == 0) { l_ls[0] = a.lut_scales[n]; l_lb[0] = a.lut_biases[n]; } }
        else for (int i = tid; i < G; i += FT) { l_ls[i] = __fmul_rn(LSK, a.lut_scales[(size_t)n * G + i]); l_lb[i] = __fmul_rn(LSK, a.lut_biases[(size_t)n * G + i]); }
    } else {
        float gscale = 0.f, gtinv = 0.f;
        if (SM == 2) {
            // One act group = the whole row: the scale needs a maximum over K, and lut_biases is ONE fp32 chain over the K/32
            // 8-table chunk sums in order (lut_ctor.cc:157,218) -- 270 dependent adds for K = 8640, a microsecond of a single
            // lane.  Neither the chunk sums nor the chain depend on the scale, so: pass 1 computes maxima AND chunk sums
            // (LUT[0] of a table is -(((x0+x1)+x2)+x3), the same adds q_table8 performs), one barrier, then lane 0 of the last
            // wave walks the chain while every other wave already builds its tables.
            float mx = 0.f;
#pragma unroll
            for (int r = 0; r < NP; ++r) {
                const int p = r * FT + tid;
                if (p < P) {
                    float x[8];
                    unpack(r, x);
                    mx = fmaxf(mx, __fadd_rn(__fadd_rn(fabsf(x[0]), fabsf(x[1])), __fadd_rn(fabsf(x[2]), fabsf(x[3]))));
                    mx = fmaxf(mx, __fadd_rn(__fadd_rn(fabsf(x[4]), fabsf(x[5])), __fadd_rn(fabsf(x[6]), fabsf(x[7]))));
                    float va = -__fadd_rn(__fadd_rn(__fadd_rn(x[0], x[1]), x[2]), x[3]);
                    float vb = -__fadd_rn(__fadd_rn(__fadd_rn(x[4], x[5]), x[6]), x[7]);
                    va = __fadd_rn(va, dpp_f<0x4E>(va));      // lane ^ 2: v0+v4 | v2+v6      (lut_ctor.cc:25-31)
                    vb = __fadd_rn(vb, dpp_f<0x4E>(vb));      //           v1+v5 | v3+v7
                    va = __fadd_rn(va, dpp_f<0xB1>(va));      // lane ^ 1: (v0+v4)+(v2+v6)
                    vb = __fadd_rn(vb, dpp_f<0xB1>(vb));      //           (v1+v5)+(v3+v7)
                    if ((p & 3) == 0) l_scr[NWV + (p >> 2)] = __fadd_rn(va, vb);
                }
            }
            mx = lut_wave_max(mx);
            if (lane == 0) l_scr[w] = mx;
            __syncthreads();
            mx = l_scr[0];
#pragma unroll
            for (int i = 1; i < NWV; ++i) mx = fmaxf(mx, l_scr[i]);
            gscale = __fdiv_rn(mx, 127.0f);
            gtinv = (gscale != 0.0f) ? __fdiv_rn(1.0f, gscale) : 0.0f;
            if (tid == FT - 64) {   // the last wave holds the fewest pairs (none when K/8 <= FT - 64)
                // the LDS reads are batched (16-byte reads, unrolled) so that only the dependent adds are serial
                float biases = 0.0f;
                const float4* cs = reinterpret_cast<const float4*>(l_scr + NWV);
                const int nc = T / 8;
                int c = 0;
#pragma unroll 4
                for (; c + 4 <= nc; c += 4) {
                    const float4 v4 = cs[c >> 2];
                    biases = __fadd_rn(__fadd_rn(__fadd_rn(__fadd_rn(biases, v4.x), v4.y), v4.z), v4.w);
                }
                for (; c < nc; ++c) biases = __fadd_rn(biases, l_scr[NWV + c]);
                l_ls[0] = gscale;
                l_lb[0] = biases;
            }
        }
#pragma unroll
        for (int r = 0; r < NP; ++r) {
            const int p = r * FT + tid;
            if (p < P) {   // T % 16 == 0: the 8 lanes of an act group are valid or invalid as a whole
                float x[8];
                unpack(r, x);
                float scales, t_scales;
                if (SM == 2) { scales = gscale; t_scales = gtinv; }
                else {
                    const float s0 = __fadd_rn(__fadd_rn(fabsf(x[0]), fabsf(x[1])), __fadd_rn(fabsf(x[2]), fabsf(x[3])));
                    const float s1 = __fadd_rn(__fadd_rn(fabsf(x[4]), fabsf(x[5])), __fadd_rn(fabsf(x[6]), fabsf(x[7])));
                    const float mx = q_half_allmax(fmaxf(s0, s1));
                    scales = div127(mx);
                    t_scales = (scales != 0.0f) ? rcp_exact(scales) : 0.0f;
                }
                uint32_t lo0, hi0, lo1, hi1;
                float La, Lb;
                lut_tables2_words<ACC == 1>(LUT_X8(x), t_scales, lo0, hi0, lo1, hi1, La, Lb);
                // tables 2p, 2p+1 = the uint4 (j4 = p & 3) of unit p >> 2
                tab[(p & 3) * tstride + (p >> 2)] = make_uint4(lo0, hi0, lo1, hi1);
                const float v = lut_chunk_sum(La, Lb);
                if (SM != 2) {
                    const float c1 = lut_group_partner(v);      // (every lane of the act group takes part)
                    if ((p & 7) == 0) {
                        l_ls[p >> 3] = __fmul_rn(LSK, scales);
                        l_lb[p >> 3] = __fmul_rn(LSK, lut_group_bias(v, c1));
                    }
                }
            }
        }
    }
    {   // zero tables for the units between K and the end of the last 64-unit step
        const uint32_t z = (ACC == 1) ? 0u : 0x80808080u;
#pragma unroll
        for (int j4 = 0; j4 < 4; ++j4)
            for (int u = nu + tid; u < nst * 64; u += FT) tab[j4 * tstride + u] = make_uint4(z, z, z, z);
        if (SM != 2)
            for (int i = G + tid; i < GP; i += FT) { l_ls[i] = 0.f; l_lb[i] = 0.f; }
    }
    QSTAMP(2);
    if (!early) {
        issue(f0); issue(f1);
        if (RING == 4) { issue(f2); issue(f3); }
    }
    __syncthreads();
    QSTAMP(3);
    if (a.lut_tap && blockIdx.x == 0) {
        for (int i = tid; i < (SM == 2 ? 1 : G); i += FT) { a.lut_tap[(size_t)n * 2 * G + i] = __fmul_rn(1.0f / LSK, l_ls[i]); a.lut_tap[(size_t)n * 2 * G + G + i] = __fmul_rn(1.0f / LSK, l_lb[i]); }
    }

    // ---- 4. stream this wave's quads -----------------------------------------------------------
    float cacc[2][BITS];
    int32_t iacc[BITS][4];
    auto reset_acc = [&]() {
#pragma unroll
        for (int pl = 0; pl < BITS; ++pl) {
            cacc[0][pl] = 0.f; cacc[1][pl] = 0.f;
#pragma unroll
            for (int be = 0; be < 4; ++be) iacc[pl][be] = 0;
        }
    };
    reset_acc();
    const int beta0 = 2 * (lane & 1);

    auto compute = [&](const WFrag<BITS>& f, int st, int Mw_m, int lq) {
        const int u = st * 64 + lane;
        if (u >= nu) return;                 // nu is even: both lanes of a pair are valid or not
        uint32_t tb[16];
#pragma unroll
        for (int j4 = 0; j4 < 4; ++j4) {
            const uint4 v = tab[j4 * tstride + u];
            tb[4 * j4] = v.x; tb[4 * j4 + 1] = v.y; tb[4 * j4 + 2] = v.z; tb[4 * j4 + 3] = v.w;
        }
        SegAcc<BITS, 0> acc;
        acc.reset();
        accumulate_tables<BITS, 0, 8>(f.wd, tb, acc);
        if (SM == 2) {
#pragma unroll
            for (int pl = 0; pl < BITS; ++pl)
#pragma unroll
                for (int be = 0; be < 4; ++be) iacc[pl][be] += acc.ps(pl, be, 8);
            return;
        }
        const int kk = u >> 1;
        const float ls = l_ls[kk], lb = l_lb[kk];
#pragma unroll
        for (int pl = 0; pl < BITS; ++pl) {
            uint32_t lo = (uint32_t)acc.a[pl], hi = (uint32_t)(acc.a[pl] >> 32);
            lo += dpp_u<0xB1>(lo);          // the two 8-table halves of the act group: lanes (l, l^1)
            hi += dpp_u<0xB1>(hi);
            const uint32_t mine = (lane & 1) ? hi : lo;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int32_t ps = 127 * 16 - (int32_t)((mine >> (16 * i)) & 0xffff);
                if (DUMP && a.dump) {
                    const int o = 4 * lq + beta0 + i;
                    if (o < Mw_m) a.dump[((size_t)n * Mw_m * BITS + mrow(o, pl, BITS)) * G + kk] = ps;
                }
                const float v = (pl == 0) ? __fmaf_rn((float)ps, ls, lb) : __fmul_rn((float)ps, ls);
                float c = __fmaf_rn(v, frag_scale<ZP>(f.sraw, SCF16, i, 0), cacc[i][pl]);
                if (ZP && pl == 0) c = __fmaf_rn(frag_scale<ZP>(f.sraw, SCF16, i, 1), __fmul_rn(2.0f, lb), c);
                cacc[i][pl] = c;
            }
        }
    };

    // ---- ACC == 1 ------------------------------------------------------------------------------
    qv4i_t bsel;
    {
        const int jrel = (lane & 15) - 4 * (lane >> 4);
        const uint32_t be = (jrel >= 0 && jrel < 4) ? (0x01u << (8 * jrel)) : 0u, bo = (jrel >= 0 && jrel < 4) ? (0xfeu << (8 * jrel)) : 0u;   // +1 | -2
        bsel = (qv4i_t){(int)be, (int)bo, (int)be, (int)bo};
    }
    uint32_t k3 = 0x03020100u;
    asm volatile("" : "+v"(k3));     // keep the selector constant in a VGPR (operand of v_and_or_b32)
    auto compute_mfma = [&](const WFrag<BITS>& f, int st, int Mw_m, int lq) {
        const int u = st * 64 + lane;
        uint32_t tb[16];
#pragma unroll
        for (int j4 = 0; j4 < 4; ++j4) {
            const uint4 v = tab[j4 * tstride + u];            // units past K read the zero tables: no contribution
            tb[4 * j4] = v.x; tb[4 * j4 + 1] = v.y; tb[4 * j4 + 2] = v.z; tb[4 * j4 + 3] = v.w;
        }
        qv4i_t c[BITS];
#pragma unroll
        for (int pl = 0; pl < BITS; ++pl) c[pl] = (qv4i_t){0, 0, 0, 0};
#pragma unroll
        for (int tp = 0; tp < 4; ++tp) {
#pragma unroll
            for (int pl = 0; pl < BITS; ++pl) {
                uint32_t pa, ma, pb, mb;
                const int qa = (2 * tp) * BITS + pl, qb = (2 * tp + 1) * BITS + pl;
                if (qa & 1) q_lookup4_pm<1>(f.wd[qa >> 1], tb[4 * tp], tb[4 * tp + 1], k3, pa, ma);
                else q_lookup4_pm<0>(f.wd[qa >> 1], tb[4 * tp], tb[4 * tp + 1], k3, pa, ma);
                if (qb & 1) q_lookup4_pm<1>(f.wd[qb >> 1], tb[4 * tp + 2], tb[4 * tp + 3], k3, pb, mb);
                else q_lookup4_pm<0>(f.wd[qb >> 1], tb[4 * tp + 2], tb[4 * tp + 3], k3, pb, mb);
                c[pl] = __builtin_amdgcn_mfma_i32_16x16x64_i8((qv4i_t){(int)pa, (int)ma, (int)pb, (int)mb}, bsel, c[pl], 0, 0, 0);
            }
        }
        if (SM == 2) {      // unified scale: keep the exact integer sum of this lane's row (lane & 3), all units
            // The MFMA results must have landed before a VALU instruction reads them (no hardware interlock: up to 18 wait states after an
            // 8-pass MFMA; with one bit-plane the compiler's hazard recogniser left the two a single wait state apart across the loop branch and
            // W1 unified-scale results were wrong).  ONE wait for all planes, behind the last MFMA of the step (the planes' chains are
            // interleaved, so the others finished earlier):
            // a wait per plane cost (BITS - 1) x 19 idle cycles per item
            if constexpr (BITS == 1) asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 3" : "+v"(c[0]));
            else if constexpr (BITS == 2) asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 3" : "+v"(c[0]), "+v"(c[1]));
            else if constexpr (BITS == 3) asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 3" : "+v"(c[0]), "+v"(c[1]), "+v"(c[2]));
            else asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 3" : "+v"(c[0]), "+v"(c[1]), "+v"(c[2]), "+v"(c[3]));
#pragma unroll
            for (int pl = 0; pl < BITS; ++pl) iacc[pl][0] += (c[pl].x + c[pl].y) + (c[pl].z + c[pl].w);
            return;
        }
        const int ub4 = st * 64 + 4 * (lane & 12) + 4 * (lane >> 4);
        const int o = 4 * lq + (lane & 3);
#pragma unroll
        for (int gi = 0; gi < 2; ++gi) {
            const int ug = ub4 + 2 * gi;
            {   // act groups past K have zero tables and zero LUT scale/bias: they add exactly 0, no guard needed
                const int kk = ug >> 1;
                const float hls = l_ls[kk], hlb = l_lb[kk];           // ls / 2, lb / 2 (HALVES)
                const bool first = (gi == 0) || (a.gs_shift >= 2);   // static register indices only: a run-time
                float sc, zr = 0.f;                                   // subscript would put sraw in scratch memory
                if (SCF16) {
                    const uint32_t wv = first ? f.sraw[0] : f.sraw[2];
                    sc = __half2float(__ushort_as_half((unsigned short)(wv & 0xffff)));
                    if (ZP) zr = __half2float(__ushort_as_half((unsigned short)(wv >> 16)));
                } else {
                    sc = __uint_as_float(first ? f.sraw[0] : f.sraw[2]);
                    if (ZP) zr = __uint_as_float(first ? f.sraw[1] : f.sraw[3]);
                }
                // Bit-planes are combined as integers before the one conversion and scale chain of the act group:
                //   sum_p alpha_p [(ps_p ls + [p = 0] lb) scale + [p = 0] zero 2 lb]        (tbl.cc:479-526, kernels.cc:1068)
                // = ((sum_p 2^p ps_p) (ls / 2) + lb / 2) scale + (2 zero) (lb / 2)          alpha_p = 2^(p-1); |sum| < 2^15
                // -- the same real number with fewer roundings (fp32 contract 1e-3; the integer sums stay the tap).
                int32_t comb = 0;
#pragma unroll
                for (int pl = BITS - 1; pl >= 0; --pl) {
                    const int32_t ps = (gi == 0) ? (c[pl].x + c[pl].y) : (c[pl].z + c[pl].w);
                    if (DUMP && a.dump && o < Mw_m && ug < nu) a.dump[((size_t)n * Mw_m * BITS + mrow(o, pl, BITS)) * G + kk] = ps;
                    comb = (pl == BITS - 1) ? ps : (int32_t)(((uint32_t)comb << 1) + (uint32_t)ps);   // Horner: v_lshl_add_u32
                }
                const float v = __fmaf_rn((float)comb, hls, hlb);
                float cc = __fmaf_rn(v, sc, cacc[0][0]);
                if (ZP) cc = __fmaf_rn(__fadd_rn(zr, zr), hlb, cc);
                cacc[0][0] = cc;
            }
        }
    };

    // reduce one quad over the 64 lanes (same-parity lanes of a row by DPP, rows by ds_bpermute), combine the
    // WPQ waves through LDS (double-buffered by iteration parity), store 4 outputs
    int parity = 0;
    // BI: the bias of output row o = 4 lq + lane (lane < 4) of matrix mi; -0.0f, the add's neutral element, for a matrix without one
    auto bias_of = [&](int mi, int o) -> float {
        if constexpr (BI) {
            const float* bp = a.bias[mi];
            return bp != nullptr ? bp[o] : -0.0f;
        } else {
            return 0.f;
        }
    };
    auto finish_quad = [&](bool have, const FusedMat& M, int lq) {
        float* red = l_red + parity * (NWV * 16);
        if (ACC == 1 && SM != 2) {   // per-group scales: fp32 partials
            float acc = 0.f;
            if (have) {
                acc = cacc[0][0];                             // planes already combined (compute_mfma)
                acc = __fadd_rn(acc, dpp_f<0x124>(acc));     // lanes with the same beta: rotate by 4, 8 within the row
                acc = __fadd_rn(acc, dpp_f<0x128>(acc));
                acc = q_xor_add_f(acc);
            }
            if (WPQ == 1) {
                const int o = 4 * lq + lane;
                if (have && lane < 4 && o < M.Mw) {
                    if constexpr (BI) acc = __fadd_rn(acc, bias_of(cc.mi, o));
                    st_out(M.C, a.out_f16, (size_t)n * M.Mw + o, acc);
                }
            } else {
                if (lane < 4) red[w * 4 + lane] = acc;
                __syncthreads();
                if (have && h == 0 && lane < 4) {
                    float t = red[w * 4 + lane];
#pragma unroll
                    for (int ww = 1; ww < WPQ; ++ww) t = __fadd_rn(t, red[(w + ww) * 4 + lane]);
                    const int o = 4 * lq + lane;
                    if (o < M.Mw) {
                        if constexpr (BI) t = __fadd_rn(t, bias_of(cc.mi, o));
                        st_out(M.C, a.out_f16, (size_t)n * M.Mw + o, t);
                    }
                }
            }
        } else if (SM != 2) {
            float part[2] = {0.f, 0.f};
            if (have) {
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    float acc = __fmul_rn(cacc[i][0], 0.5f);
#pragma unroll
                    for (int pl = 1; pl < BITS; ++pl) acc = __fadd_rn(acc, __fmul_rn(cacc[i][pl], alpha_of(pl)));
                    acc = __fadd_rn(acc, dpp_f<0x4E>(acc));      // lane ^ 2
                    acc = __fadd_rn(acc, dpp_f<0x124>(acc));     // rotate by 4, 8 within the 16-lane row
                    acc = __fadd_rn(acc, dpp_f<0x128>(acc));
                    acc = q_xor_add_f(acc);
                    part[i] = acc;
                }
            }
            if (WPQ == 1) {
                if (have && lane < 2) {
                    const int o = 4 * lq + 2 * lane;
                    if (o < M.Mw) st_out(M.C, a.out_f16, (size_t)n * M.Mw + o, part[0]);
                    if (o + 1 < M.Mw) st_out(M.C, a.out_f16, (size_t)n * M.Mw + o + 1, part[1]);
                }
            } else {
                if (lane < 2) { red[w * 4 + 2 * lane] = part[0]; red[w * 4 + 2 * lane + 1] = part[1]; }
                __syncthreads();
                if (have && h == 0 && lane < 4) {
                    float t = red[w * 4 + lane];
#pragma unroll
                    for (int ww = 1; ww < WPQ; ++ww) t = __fadd_rn(t, red[(w + ww) * 4 + lane]);
                    const int o = 4 * lq + lane;
                    if (o < M.Mw) st_out(M.C, a.out_f16, (size_t)n * M.Mw + o, t);
                }
            }
        } else {
            int32_t* redi = reinterpret_cast<int32_t*>(red);
            int32_t tot[BITS];
#pragma unroll
            for (int pl = 0; pl < BITS; ++pl) {
                if (ACC == 1) {       // every lane holds a partial of row lane & 3: rotate by 4, 8 within the row, then rows
                    uint32_t v = have ? (uint32_t)iacc[pl][0] : 0u;
                    v += dpp_u<0x124>(v);
                    v += dpp_u<0x128>(v);
                    v = q_xor_add_u(v);
                    tot[pl] = (int32_t)v;
                } else {
                    int32_t mine = 0;
#pragma unroll
                    for (int be = 0; be < 4; ++be) {
                        int32_t v = have ? iacc[pl][be] : 0;
#pragma unroll
                        for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
                        if (lane == be) mine = v;
                    }
                    tot[pl] = mine;
                }                     // lane be (< 4) holds row be's integer sum of this wave
            }
            if (WPQ > 1) {
                if (lane < 4)
#pragma unroll
                    for (int pl = 0; pl < BITS; ++pl) redi[(w * 4 + lane) * 4 + pl] = tot[pl];
                __syncthreads();
            }
            if (have && h == 0 && lane < 4) {
                const int o = 4 * lq + lane;
                if (o < M.Mw) {
                    float acc = 0.f;
#pragma unroll
                    for (int pl = 0; pl < BITS; ++pl) {
                        int32_t cb = tot[pl];
                        if (WPQ > 1)
#pragma unroll
                            for (int ww = 1; ww < WPQ; ++ww) cb += redi[((w + ww) * 4 + lane) * 4 + pl];
                        if (DUMP && a.dump) a.dump[(size_t)n * M.Mw * BITS + mrow(o, pl, BITS)] = cb;
                        const float t = __fmul_rn((float)cb, alpha_of(pl));
                        acc = (pl == 0) ? t : __fadd_rn(acc, t);
                    }
                    const float v = __fadd_rn(__fmul_rn(acc, l_ls[0]), __fmul_rn(l_lb[0], 0.5f));
                    st_out(M.C, a.out_f16, (size_t)n * M.Mw + o, __fmul_rn(v, ld_scale(M.SC, a.sc_f16, o / (M.Mw / s.m_groups))));
                }
            }
        }
        parity ^= 1;
        reset_acc();
    };

    // The fragment ring is consumed in issue order.  The (quad, step) work list of this wave is walked by one
    // cursor in a loop unrolled over the ring, so every fragment has a fixed role in the loop body (a run-time ring
    // position makes the compiler merge four control-flow paths with ~40 register copies per step).  A quad is
    // closed (reduce + store, workgroup barrier for WPQ > 1) when the cursor leaves it; every wave closes the
    // same number of quads, with or without work, so the barriers inside finish_quad stay matched.
    int c_it = 0, c_st = h, lq = 0;
    bool have = slot0 < total_q && h < nst;
    if (have) { seek(cc, slot0); lq = slot0 - cc.base; }
    if (blockIdx.x * IPI < total_q) {      // uniform: this workgroup has at least one quad iteration
#define QSTEP(F)                                                                                              \
        while (!(have && c_st < nst)) {                                                                       \
            if (c_it == 0) QSTAMP(4);                                                                         \
            finish_quad(have, cc.m, lq);                                                                      \
            if (c_it == 0) QSTAMP(5);                                                                         \
            ++c_it;                                                                                           \
            if (blockIdx.x * IPI + c_it * stride >= total_q) goto q_done;                                     \
            const int gq = slot0 + c_it * stride;                                                             \
            have = gq < total_q && h < nst;                                                                   \
            if (have) { seek(cc, gq); lq = gq - cc.base; }                                                                   \
            c_st = h;                                                                                         \
        }                                                                                                     \
        if (ACC == 1) compute_mfma(F, c_st, cc.m.Mw, lq); else compute(F, c_st, cc.m.Mw, lq);                   \
        issue(F);                                                                                             \
        c_st += WPQ;
        for (;;) {
            QSTEP(f0)
            QSTEP(f1)
            if (RING == 4) {
                QSTEP(f2)
                QSTEP(f3)
            }
        }
#undef QSTEP
    }
q_done:
    QSTAMP(6);
}

// ---------------------------------------------------------------------------------------------
#if !defined(TMAC_QUAD_BITS) || !defined(TMAC_QUAD_SCF16)
#error "compile with -DTMAC_QUAD_BITS=1..4 -DTMAC_QUAD_SCF16=0|1 (one translation unit per combination keeps the build parallel)"
#endif
constexpr bool QSCF16 = TMAC_QUAD_SCF16 != 0;   // weight scales stored as fp16 (1) / fp32 (0): a kernel template parameter

// This unit's launcher (declared in tmac_kernels.h; the overloads of launch_gemv_quad, tmac_launch.cpp, plan and pick the unit): select
// the instantiation the plan names and launch it.  Which instantiations exist is quad_inst_exists (tmac_launch_plan.h) -- the selector
// instantiates what passes it, so the predicate is the list of kernels this unit emits; the planner never names another.
template <int BITS, bool SCF16, class Args>
hipError_t launch_gemv_quad_unit(const Args& a, const QuadPlan& p, int N, hipStream_t st) {
    constexpr bool BI = std::is_same_v<Args, FusedBiasArgs> || std::is_same_v<Args, FusedXfBiasArgs>;
    constexpr bool XF = std::is_same_v<Args, FusedXfArgs> || std::is_same_v<Args, FusedXfBiasArgs>, GA = std::is_same_v<Args, FusedPermArgs>;
    if (p.xf != XF || p.ga != GA || p.bi != BI || ((XF || GA) && N != 1)) return hipErrorInvalidValue;
    const dim3 g(p.gx, N), b(p.ft);
    // scale flavour: unified scale (SM 2: one scalar read per output, the dtype stays a run-time flag -- fp32 unit only), or per-group scales
    // with / without zero points
    auto flavour = [&](auto&& f) {
        if (a.s.m_groups >= 1) {
            if constexpr (SCF16) return hipErrorInvalidValue;
            else return f(std::false_type{}, std::integral_constant<int, 2>{});
        }
        return sel_bool(a.s.zero_point != 0, [&](auto ZP) { return f(ZP, std::integral_constant<int, 0>{}); });
    };
    return flavour([&](auto ZP, auto SM) { return sel_int<512, 768, 1024>(p.ft, [&](auto FT) { return sel_int<1, 2, 3, 4>(p.wpq, [&](auto WPQ) {
        if constexpr (!quad_config_exists(FT, WPQ) || ((XF || GA || BI) && !quad_xf_covered(FT, WPQ))) return hipErrorInvalidValue;
        else return sel_int<2, 6>(p.nr, [&](auto NR) { return sel_bool(p.early, [&](auto EARLY) {
            if constexpr (BI) {      // per-group scales; transformed: NORM and the silu GLU (no GN, no GT); plain: the LUT built or copied
                if (p.gn || p.gt || p.dump || p.acc != 1) return hipErrorInvalidValue;
                if constexpr (SM != 0) return hipErrorInvalidValue;
                else if constexpr (XF) {
                    if constexpr (!quad_bi_inst_exists(1, NR, FT, WPQ, EARLY, true)) return hipErrorInvalidValue;
                    else return launch_lds(k_gemv_quad<BITS, ZP, 0, 1, NR, FT, WPQ, false, 1, SCF16, EARLY, true, false, false, false, true>, g, b, p.lds_bytes, st, a);
                } else return sel_bool(p.lutsrc != 0, [&](auto LUTSRC) {
                    if constexpr (!quad_bi_inst_exists(LUTSRC, NR, FT, WPQ, EARLY, false)) return hipErrorInvalidValue;
                    else return launch_lds(k_gemv_quad<BITS, ZP, 0, LUTSRC, NR, FT, WPQ, false, 1, SCF16, EARLY, false, false, false, false, true>, g, b, p.lds_bytes, st, a);
                });
            } else if constexpr (XF) {
                return sel_bool(p.gn, [&](auto GN) { return sel_bool(p.gt, [&](auto GT) {
                    if constexpr (!quad_inst_exists(1, NR, FT, WPQ, false, 1, EARLY, true)) return hipErrorInvalidValue;
                    else return launch_lds(k_gemv_quad<BITS, ZP, SM, 1, NR, FT, WPQ, false, 1, SCF16, EARLY, true, GN, GT>, g, b, p.lds_bytes, st, a);
                }); });
            } else if constexpr (GA) {
                if constexpr (SM != 0 || !quad_ga_inst_exists(NR, FT, WPQ, EARLY)) return hipErrorInvalidValue;
                else return launch_lds(k_gemv_quad<BITS, ZP, 0, 1, NR, FT, WPQ, false, 1, SCF16, EARLY, false, false, false, true>, g, b, p.lds_bytes, st, a);
            } else {
                return sel_bool(p.lutsrc != 0, [&](auto LUTSRC) { return sel_bool(p.dump, [&](auto DUMP) { return sel_bool(p.acc != 0, [&](auto ACC) {
                    if constexpr (!quad_inst_exists(LUTSRC, NR, FT, WPQ, DUMP, ACC, EARLY, false)) return hipErrorInvalidValue;
                    else return launch_lds(k_gemv_quad<BITS, ZP, SM, LUTSRC, NR, FT, WPQ, DUMP, ACC, SCF16, EARLY>, g, b, p.lds_bytes, st, a);
                }); }); });
            }
        }); });
    }); }); });
}
// (the bias instantiations in objects of their own, -DTMAC_QUAD_BI_TU=1: the ones above hold exactly the kernels they held before, and the
// build stays parallel)
#if defined(TMAC_QUAD_BI_TU) && TMAC_QUAD_BI_TU
template hipError_t launch_gemv_quad_unit<TMAC_QUAD_BITS, QSCF16, FusedBiasArgs>(const FusedBiasArgs&, const QuadPlan&, int, hipStream_t);
template hipError_t launch_gemv_quad_unit<TMAC_QUAD_BITS, QSCF16, FusedXfBiasArgs>(const FusedXfBiasArgs&, const QuadPlan&, int, hipStream_t);
#else
template hipError_t launch_gemv_quad_unit<TMAC_QUAD_BITS, QSCF16, FusedArgs>(const FusedArgs&, const QuadPlan&, int, hipStream_t);
template hipError_t launch_gemv_quad_unit<TMAC_QUAD_BITS, QSCF16, FusedXfArgs>(const FusedXfArgs&, const QuadPlan&, int, hipStream_t);
template hipError_t launch_gemv_quad_unit<TMAC_QUAD_BITS, QSCF16, FusedPermArgs>(const FusedPermArgs&, const QuadPlan&, int, hipStream_t);
#endif

}  // namespace tmac
