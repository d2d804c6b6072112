// tmac_prefill_lut.hip — the LUT builders of the N > 1 routes that work pair-wise (k_preprocess_pairs, k_preprocess_pairs_row) and the row
// pass of the vector transforms in front of them (k_xf_rows, k_xf_rows_tap), with their launchers.  The third builder, k_lut_image, lives
// with the GEMM that streams its image (tmac_gemm2.hip).  DESIGN.md 4.6, 4.8.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>

#include "tmac_core.h"
#include "tmac_kernels.h"
#include "tmac_quad_core.h"
#include "tmac_select.h"

namespace tmac {

// ---------------------------------------------------------------------------------------------
// Prefill LUT build for the fused entry point: the quad kernel's build phase as a kernel of its own.  One lane builds
// the two tables of pair p (8 activations, one 16-byte fp16 load) of activation row n with the packed-fp32 sequence of
// q_table8, the act group (64 activations = 8 lanes) shares its abs-max by DPP, and the result goes straight into the
// unit-major half-table image the one-hot GEMM stages from (same bytes as k_preprocess writes there; QLUT, scales and
// biases bit-identical to lut_ctor.cc: the pieces of tmac_lut_build.h).  k_preprocess keeps one workgroup per
// act group with 16 of 64 lanes building tables and writes three layouts; this one writes the image only.
// ---------------------------------------------------------------------------------------------
// XF (both pair builds; tmac_hip_qgemm_fused_xf_rows_dev): x is the vector transform of (row n, pair p) -- xf_rows_x8, tmac_quad_core.h --
// and the kernel takes an XfRowsArgs behind its own arguments; off, there is no such argument and the code is what it was.
template <bool F16, bool ALL, bool XF = false, class... XA>
__global__ __launch_bounds__(256) void k_preprocess_pairs(const void* __restrict__ B, uint4* __restrict__ qlut_lds,
                                                          float* __restrict__ lut_scales, float* __restrict__ lut_biases,
                                                          int K, int tstride, uint4* __restrict__ qlut_ref,
                                                          uint2* __restrict__ qlut_dev, size_t qdev_u4_per_row, XA... xa) {
    const int P = K / 8, G = K / 64, n = blockIdx.y;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;                     // P % 8 == 0: the 8 lanes of an act group leave together
    float x[8];
    if constexpr (XF) {
        xf_rows_x8(xf_rows_arg(xa...), B, F16, K, n, p, x);
    } else {
        lut_ld8(B, F16, (size_t)n * K, p, x);
    }
    float scales, t_scales, La, Lb;
    lut_group_scale(LUT_X8(x), scales, t_scales);
    const uint4 t = lut_tables2<false>(LUT_X8(x), t_scales, La, Lb);     // biased bytes, as the image holds them
    qlut_lds[((size_t)n * 4 + (p & 3)) * tstride + (p >> 2)] = t;
    if (ALL) lut_store_ref_dev(t, K, n, p, qlut_ref, qlut_dev, qdev_u4_per_row);      // the workspace's other two layouts (tmac_hip_preprocessor_dev serves every consumer)
    const float v = lut_chunk_sum(La, Lb);
    const float c1 = lut_group_partner(v);
    if ((p & 7) == 0) {
        lut_scales[(size_t)n * G + (p >> 3)] = scales;
        lut_biases[(size_t)n * G + (p >> 3)] = lut_group_bias(v, c1);
    }
}

// The same for one act group per row (act_group_size = K, the unified-scale / BitNet flavour): a workgroup owns an
// activation row.  Pass 1: abs-max of the row and the 8-table chunk sums of lut_biases (neither depends on the scale);
// then one lane walks the reference's sequential fp32 chain over the chunk sums (lut_ctor.cc:157,218) while the other
// waves quantise their tables -- the build phase of k_gemv_quad's SM == 2 path as a kernel of its own.
// (The load of 8 and the ALL block stay in this kernel's own words: through lut_ld8 / lut_store_ref_dev two instantiations changed their
// instruction count, profiles/r18_lut_build_refactor.txt.)
template <bool F16, bool ALL, int PT, bool XF = false, class... XA>
__global__ __launch_bounds__(PT) void k_preprocess_pairs_row(const void* __restrict__ B, uint4* __restrict__ qlut_lds,
                                                               float* __restrict__ lut_scales, float* __restrict__ lut_biases,
                                                               int K, int tstride, uint4* __restrict__ qlut_ref,
                                                               uint2* __restrict__ qlut_dev, size_t qdev_u4_per_row,
                                                               uint4* __restrict__ bimg, float* __restrict__ colv, int Npad, XA... xa) {
    extern __shared__ float prs[];          // [PT/64] wave maxima | [K/32] chunk sums
    constexpr int NWV = PT / 64;
    const int P = K / 8, n = blockIdx.x, tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    float* l_mx = prs;
    float* l_cs = prs + NWV;
    int* l_hs = reinterpret_cast<int*>(prs + NWV + K / 32);      // sum of all signed half-table entries of the row (LUT image only)
    if (tid == 0) *l_hs = 0;
    constexpr int NPR = 3;                   // pairs per thread: K <= 24 * PT
    float x[NPR][8];
    float mx = 0.f;
#pragma unroll
    for (int r = 0; r < NPR; ++r) {
        const int p = r * PT + tid;
        if (p < P) {
            if constexpr (XF) {
                xf_rows_x8(xf_rows_arg(xa...), B, F16, K, n, p, x[r]);
            } else if (F16) {
                const uint4 v = reinterpret_cast<const uint4*>(reinterpret_cast<const __half*>(B) + (size_t)n * K)[p];
                const uint32_t rr[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const __half2 hh = *reinterpret_cast<const __half2*>(&rr[i]);
                    x[r][2 * i] = __low2float(hh); x[r][2 * i + 1] = __high2float(hh);
                }
            } else {
                const float4* src = reinterpret_cast<const float4*>(reinterpret_cast<const float*>(B) + (size_t)n * K) + 2 * (size_t)p;
                const float4 a0 = src[0], a1 = src[1];
                x[r][0] = a0.x; x[r][1] = a0.y; x[r][2] = a0.z; x[r][3] = a0.w; x[r][4] = a1.x; x[r][5] = a1.y; x[r][6] = a1.z; x[r][7] = a1.w;
            }
            mx = fmaxf(mx, lut_abssum4(x[r][0], x[r][1], x[r][2], x[r][3]));
            mx = fmaxf(mx, lut_abssum4(x[r][4], x[r][5], x[r][6], x[r][7]));
            float va = lut_lut0(x[r][0], x[r][1], x[r][2], x[r][3]), vb = lut_lut0(x[r][4], x[r][5], x[r][6], x[r][7]);
            lut_chunk_fold(va, vb);
            if ((p & 3) == 0) l_cs[p >> 2] = __fadd_rn(va, vb);
        }
    }
    mx = lut_wave_max(mx);
    if (lane == 0) l_mx[w] = mx;
    __syncthreads();
    mx = l_mx[0];
#pragma unroll
    for (int i = 1; i < NWV; ++i) mx = fmaxf(mx, l_mx[i]);
    float gscale, gtinv;
    lut_scale<true>(mx, gscale, gtinv);
    if (tid == PT - 64) {
        float biases = 0.0f;
        const int nc = K / 32;
        for (int c = 0; c < nc; ++c) biases = __fadd_rn(biases, l_cs[c]);
        lut_scales[n] = gscale;
        lut_biases[n] = biases;
        if (colv) { colv[n] = gscale; colv[Npad + n] = biases; }      // the layout k_gemm_planes_us reads (tmac_gemm2.hip)
    }
    int hsum = 0;
#pragma unroll
    for (int r = 0; r < NPR; ++r) {
        const int p = r * PT + tid;
        if (p < P) {
            float La, Lb;
            const uint4 t = lut_tables2<false>(LUT_X8(x[r]), gtinv, La, Lb);
            const uint32_t lo0 = t.x, hi0 = t.y, lo1 = t.z, hi1 = t.w;
            qlut_lds[((size_t)n * 4 + (p & 3)) * tstride + (p >> 2)] = t;
            if (bimg) {  // signed half tables, [unit][pair][n]: what the plane-combined GEMM streams
                bimg[(size_t)p * Npad + n] = make_uint4(lo0 ^ 0x80808080u, hi0 ^ 0x80808080u, lo1 ^ 0x80808080u, hi1 ^ 0x80808080u);
                // the 16 entries are biased bytes U = entry + 128: sum of the bytes - 16 * 128
                hsum += (int)__builtin_amdgcn_sad_u8(lo0, 0u, __builtin_amdgcn_sad_u8(hi0, 0u, __builtin_amdgcn_sad_u8(lo1, 0u, __builtin_amdgcn_sad_u8(hi1, 0u, 0u)))) - 2048;
            }
            if (ALL) {
                const int seg = p >> 3, j8 = p & 7;
                *reinterpret_cast<uint4*>(qlut_dev + ((size_t)n * qdev_u4_per_row + qlut_dev_u4_index(seg, j8)) * 2) = make_uint4(lo0, hi0, lo1, hi1);
                const uint32_t sg = 0x80808080u, rev = 0x00010203u;
                const uint32_t n0l = __builtin_amdgcn_perm(0u, 0x01010100u - lo0, rev), n0h = __builtin_amdgcn_perm(0u, 0x01010100u - hi0, rev);
                const uint32_t n1l = __builtin_amdgcn_perm(0u, 0x01010100u - lo1, rev), n1h = __builtin_amdgcn_perm(0u, 0x01010100u - hi1, rev);
                uint4* rp = qlut_ref + ((size_t)n * (K / 4) + 2 * (size_t)p);
                rp[0] = make_uint4(lo0 ^ sg, hi0 ^ sg, n0h ^ sg, n0l ^ sg);
                rp[1] = make_uint4(lo1 ^ sg, hi1 ^ sg, n1h ^ sg, n1l ^ sg);
            }
        }
    }
    if (colv) {   // (uniform) the row's entry sum, int32 bits: what the +7 / +15 operand bytes of 3- / 4-bit rows add per unit of it
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) hsum += __shfl_xor(hsum, off);
        if (lane == 0) atomicAdd(l_hs, hsum);
        __syncthreads();
        if (tid == 0) colv[2 * (size_t)Npad + n] = __int_as_float(*l_hs);
    }
}

// ---------------------------------------------------------------------------------------------
// Vector transforms for N > 1 rows: the row pass in front of an XF LUT build.  One workgroup per activation row.  NORM: t = fp32(in)
// + residual (xf_rows_t8: the add the builders repeat), t to residual_out -- pair p of row n has exactly one writer, thread p mod 256 of
// workgroup n -- and, with gamma, r[n] = rsq(fma(sum t^2, rcp(K), eps)), k_gemv_quad's expression.  The order of the sum is a function of K
// alone: thread j adds its pairs j, j + 256, ... element by element (fma), the wave's 64 sums fold by xor 32, 16, ... 1, the four wave
// sums are added in wave order.  Neither N, the row's index nor any launch knob enters: a row's r is the same in every call.
// GLU_NORM (kind 4): t = g = gate(in) * in2 (xf_rows_g8: the product the builders repeat), summed in the same order; r[n] is all it writes.
// ---------------------------------------------------------------------------------------------
constexpr int XF_ROWS_PT = 256;
template <bool F16, class XA = XfRowsArgs>
__global__ __launch_bounds__(XF_ROWS_PT) void k_xf_rows(XA a, const void* __restrict__ B, float* __restrict__ r_out, int K) {
    __shared__ float l_ss[XF_ROWS_PT / 64];
    const int P = K / 8, n = blockIdx.x, tid = threadIdx.x;
    float ss = 0.f;
    for (int p = tid; p < P; p += XF_ROWS_PT) {
        float t[8];
        if (a.kind == 4) xf_rows_g8(a, B, F16, K, n, p, t);
        else xf_rows_t8(a, B, F16, K, n, p, t);
        if (a.residual_out != nullptr) {
            float4* ro = reinterpret_cast<float4*>(a.residual_out + (size_t)n * K) + 2 * (size_t)p;
            ro[0] = make_float4(t[0], t[1], t[2], t[3]);
            ro[1] = make_float4(t[4], t[5], t[6], t[7]);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) ss = __fmaf_rn(t[i], t[i], ss);
    }
    if (r_out == nullptr) return;           // (uniform)
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) ss = __fadd_rn(ss, __shfl_xor(ss, off, 64));
    if ((tid & 63) == 0) l_ss[tid >> 6] = ss;
    __syncthreads();
    if (tid == 0) {
        float tot = 0.f;
#pragma unroll
        for (int w = 0; w < XF_ROWS_PT / 64; ++w) tot = __fadd_rn(tot, l_ss[w]);
        r_out[n] = __builtin_amdgcn_rsqf(__fmaf_rn(tot, __builtin_amdgcn_rcpf((float)K), a.eps));
    }
}
// the fp32 x [N][K] the XF builders consume (tmac_hip_debug_xf_rows): a store around xf_rows_x8
template <bool F16, class XA = XfRowsArgs>
__global__ __launch_bounds__(256) void k_xf_rows_tap(XA a, const void* __restrict__ B, float* __restrict__ x_out, int K) {
    const int P = K / 8, n = blockIdx.y;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    float x[8];
    xf_rows_x8(a, B, F16, K, n, p, x);
    float4* xo = reinterpret_cast<float4*>(x_out + (size_t)n * K) + 2 * (size_t)p;
    xo[0] = make_float4(x[0], x[1], x[2], x[3]);
    xo[1] = make_float4(x[4], x[5], x[6], x[7]);
}

// ---- launchers ----------------------------------------------------------------------------------------------------------------------
hipError_t launch_xf_rows(const XfRowsGateArgs& xf, const void* B, int act_f16, float* r_out, int K, int N, hipStream_t st) {
    if (K % 64 != 0 || N < 1 || (xf.kind != 1 && xf.kind != 4) || (r_out == nullptr && xf.residual_out == nullptr)) return hipErrorInvalidValue;
    if (xf.kind == 4 && (!xf.in2 || !xf.gamma || !r_out || xf.residual || xf.residual_out)) return hipErrorInvalidValue;
    if (xf.gate < XF_GATE_SILU || xf.gate > XF_GATE_GELU) return hipErrorInvalidValue;
    return sel_bool(act_f16 != 0, [&](auto F16) { return sel_xf_block(xf, [&](const auto& blk) {
        using T = std::decay_t<decltype(blk)>;
        return launch_lds(k_xf_rows<F16.value, T>, dim3(N), dim3(XF_ROWS_PT), 0, st, blk, B, r_out, K);
    }); });
}
hipError_t launch_xf_rows_tap(const XfRowsGateArgs& xf, const void* B, int act_f16, float* x_out, int K, int N, hipStream_t st) {
    if (K % 64 != 0 || N < 1 || N > 65535 || (xf.kind != 1 && xf.kind != 2 && xf.kind != 4) || !x_out) return hipErrorInvalidValue;
    if (xf.gate < XF_GATE_SILU || xf.gate > XF_GATE_GELU) return hipErrorInvalidValue;
    return sel_bool(act_f16 != 0, [&](auto F16) { return sel_xf_block(xf, [&](const auto& blk) {
        using T = std::decay_t<decltype(blk)>;
        return launch_lds(k_xf_rows_tap<F16.value, T>, dim3((K / 8 + 255) / 256, N), dim3(256), 0, st, blk, B, x_out, K);
    }); });
}

hipError_t launch_preprocess_pairs_row(const void* B, int act_f16, void* qlut_lds, float* lut_scales, float* lut_biases, int K, int N,
                                       int8_t* qlut_ref, void* qlut_dev, size_t qdev_u4_per_row, void* bimg, float* colv, int Npad, hipStream_t st,
                                       const XfRowsGateArgs* xf) {
    constexpr int PT = 512;
    if (K % 64 != 0 || N < 1 || K > 24 * PT || ((qlut_ref == nullptr) != (qlut_dev == nullptr))) return hipErrorInvalidValue;
    if (xf && qlut_ref) return hipErrorInvalidValue;
    const int tstride = (((K / 32) + 15) & ~15) + 1;
    const size_t shmem = sizeof(float) * (PT / 64 + K / 32 + 1);
    const dim3 g(N), b(PT);
    return sel_bool(act_f16 != 0, [&](auto F16) {
        if (xf) return sel_xf_block(*xf, [&](const auto& blk) {
            using T = std::decay_t<decltype(blk)>;
            return launch_lds(k_preprocess_pairs_row<F16.value, false, PT, true, T>, g, b, shmem, st, B, (uint4*)qlut_lds, lut_scales, lut_biases, K, tstride,
                              (uint4*)nullptr, (uint2*)nullptr, (size_t)0, (uint4*)bimg, colv, Npad, blk);
        });
        return sel_bool(qlut_ref != nullptr, [&](auto ALL) {
            return launch_lds(k_preprocess_pairs_row<F16.value, ALL.value, PT>, g, b, shmem, st, B, (uint4*)qlut_lds, lut_scales, lut_biases, K, tstride,
                              (uint4*)qlut_ref, (uint2*)qlut_dev, qdev_u4_per_row, (uint4*)bimg, colv, Npad);
        });
    });
}

hipError_t launch_preprocess_pairs(const void* B, int act_f16, void* qlut_lds, float* lut_scales, float* lut_biases, int K, int N,
                                   int8_t* qlut_ref, void* qlut_dev, size_t qdev_u4_per_row, hipStream_t st, const XfRowsGateArgs* xf, const int32_t* perm) {
    if (K % 64 != 0 || N < 1 || ((qlut_ref == nullptr) != (qlut_dev == nullptr))) return hipErrorInvalidValue;
    if ((xf && qlut_ref) || (xf && perm)) return hipErrorInvalidValue;
    const int tstride = (((K / 32) + 15) & ~15) + 1;
    const dim3 g((K / 8 + 255) / 256, N), b(256);
    return sel_bool(act_f16 != 0, [&](auto F16) {
        // act-order: the gathered build, the image alone or every layout (tmac_hip_preprocessor_perm_dev)
        if (perm) return sel_bool(qlut_ref != nullptr, [&](auto ALL) {
            return launch_lds(k_preprocess_pairs<F16.value, ALL.value, true, GatherRowsArgs>, g, b, 0, st, B, (uint4*)qlut_lds, lut_scales, lut_biases, K, tstride,
                              (uint4*)qlut_ref, (uint2*)qlut_dev, qdev_u4_per_row, GatherRowsArgs{perm});
        });
        if (xf) return sel_xf_block(*xf, [&](const auto& blk) {
            using T = std::decay_t<decltype(blk)>;
            return launch_lds(k_preprocess_pairs<F16.value, false, true, T>, g, b, 0, st, B, (uint4*)qlut_lds, lut_scales, lut_biases, K, tstride,
                              (uint4*)nullptr, (uint2*)nullptr, (size_t)0, blk);
        });
        return sel_bool(qlut_ref != nullptr, [&](auto ALL) {
            return launch_lds(k_preprocess_pairs<F16.value, ALL.value>, g, b, 0, st, B, (uint4*)qlut_lds, lut_scales, lut_biases, K, tstride,
                              (uint4*)qlut_ref, (uint2*)qlut_dev, qdev_u4_per_row);
        });
    });
}

}  // namespace tmac
