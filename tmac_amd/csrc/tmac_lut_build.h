// tmac_lut_build.h — the LUT constructor on the device, written once: every kernel that builds tables is made of these pieces and decides
// only where the result is stored.  A few sites keep single steps in their own words, because through the shared piece the compiler
// scheduled some of their instantiations differently; profiles/r18_lut_build_refactor.txt lists them per piece and per kernel:
// k_gemv_quad (fp16 unpack, pass 1 of the unified-scale path with its two divisions, the act-group scale), k_decode_chain (fp16 unpack,
// the act-group scale), k_preprocess_pairs_row (the load of 8, the reference and device layouts).
//
// What the reference does per act group (lut_ctor.cc:120-215) and where it is here, 8 activations x[0..7] (two tables) per lane:
//   :240-256  partial_max: abs-max of the act group over the tables' (|x0|+|x1|)+(|x2|+|x3|), divided by 127 -> lut_abssum4, lut_absmax8;
//             the maximum over the lanes of the act group is q_half_allmax (8 lanes = 64 activations) or, one act group per row, the
//             row's (lut_wave_max, then across waves at the site)
//   :124-125  scales as partial_max left it, t_scales = scales ? 1 / scales : 0, IEEE divisions              -> lut_scale
//   :133-155  the odd entries ((x0 +- x1) +- x2) +- x3 in that association; entry 15 - j is minus entry j, so a table is kept as
//             its 8 entries of one sign
//   :159-178  times t_scales, rounded to nearest even, saturated to int8                                     -> q_table8, lut_tables2
//   :157      lut_biases: LUT[0] of each table (= -L15), summed per chunk of 8 tables by _mm256_addv_ps (:25-31) as
//             ((v0+v4)+(v2+v6)) + ((v1+v5)+(v3+v7)); the 4 lanes of a chunk hold (v0,v1), (v2,v3), (v4,v5), (v6,v7)
//                                                                                                            -> lut_chunk_fold, lut_chunk_sum
//   :122,157,218  and the chunk sums added to a zero-initialised accumulator in order: (0 + c0) + c1 for an act group of 64 (two
//             chunks: lut_group_partner, lut_group_bias); one chain over all K / 32 chunks for one act group per row (walked at the site)
// One act group per row (unified scale, qgemm.py:93-96): neither the chunk sums nor the chain depend on the scale, so pass 1 (lut_row_pass1)
// forms the lane's maximum AND the chunk sums straight from x -- LUT[0] = -(((x0+x1)+x2)+x3), the adds q_table8 performs.
// The arithmetic is fp32 with every operation rounded on its own (-ffp-contract=off); tmac_fastdiv.h proves div127 / rcp_exact equal
// to the divisions for every input.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>

#include "tmac_dev.h"
#include "tmac_fastdiv.h"
#include "tmac_layout.h"

namespace tmac {

typedef float qv2f __attribute__((ext_vector_type(2)));

// The pieces take the 8 activations of a pair by value (LUT_X8(x) spells out x[0] .. x[7]) and hand results back as values or through
// scalar references, like q_table8; the loaders return a vector of 8 floats.  Inlined, that form is the text the sites used to carry.
#define LUT_X8(x) (x)[0], (x)[1], (x)[2], (x)[3], (x)[4], (x)[5], (x)[6], (x)[7]

// ---- the 8 activations of a pair -------------------------------------------------------------------------------------------
typedef float lut_f32x8 __attribute__((ext_vector_type(8)));
// 16 bytes of fp16 (4 words) / 32 bytes of fp32 (8 words), already loaded, as fp32
__device__ __forceinline__ lut_f32x8 lut_unpack_f16v(const uint32_t* w) {
    lut_f32x8 r;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const __half2 hh = *reinterpret_cast<const __half2*>(&w[i]);
        r[2 * i] = __low2float(hh); r[2 * i + 1] = __high2float(hh);
    }
    return r;
}
// Pair p behind element `off` of an fp16 / fp32 operand (off = n * K for row n of an [N][K] one), loaded and converted
__device__ __forceinline__ lut_f32x8 lut_ld8v(const void* base, bool f16, size_t off, int p) {
    if (!f16) {
        const float4* src = reinterpret_cast<const float4*>(reinterpret_cast<const float*>(base) + off) + 2 * (size_t)p;
        const float4 a0 = src[0], a1 = src[1];
        return (lut_f32x8){a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
    } else {
        const uint4 v = reinterpret_cast<const uint4*>(reinterpret_cast<const __half*>(base) + off)[p];
        const uint32_t r[4] = {v.x, v.y, v.z, v.w};
        return lut_unpack_f16v(r);
    }
}
__device__ __forceinline__ void lut_ld8(const void* base, bool f16, size_t off, int p, float (&x)[8]) {
    const lut_f32x8 r = lut_ld8v(base, f16, off, p);
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = r[i];
}

// ---- abs-max and scale -----------------------------------------------------------------------------------------------------
__device__ __forceinline__ float lut_abssum4(float x0, float x1, float x2, float x3) {
    return __fadd_rn(__fadd_rn(fabsf(x0), fabsf(x1)), __fadd_rn(fabsf(x2), fabsf(x3)));
}
__device__ __forceinline__ float lut_absmax8(float x0, float x1, float x2, float x3, float x4, float x5, float x6, float x7) {
    const float s0 = lut_abssum4(x0, x1, x2, x3);
    const float s1 = lut_abssum4(x4, x5, x6, x7);
    return fmaxf(s0, s1);
}
// max over the 16 lanes of a DPP row, result in every lane.  v_max_f32 with a DPP source operand: fmaxf() through
// update_dpp costs a v_mov_dpp plus canonicalising v_max pairs (5 instructions per step instead of 1).  The s_nop
// covers the VALU-write -> DPP-read hazard, which the compiler does not track through inline asm.
__device__ __forceinline__ float q_row_allmax(float v) {
    asm("s_nop 1\n\tv_max_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\tv_max_f32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\tv_max_f32_dpp %0, %0, %0 row_half_mirror row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\tv_max_f32_dpp %0, %0, %0 row_mirror row_mask:0xf bank_mask:0xf"
        : "+v"(v));
    return v;
}
// max over the 8 lanes of half a DPP row (the two quads of one act group when a lane holds two tables)
__device__ __forceinline__ float q_half_allmax(float v) {
    asm("s_nop 1\n\tv_max_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\tv_max_f32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\tv_max_f32_dpp %0, %0, %0 row_half_mirror row_mask:0xf bank_mask:0xf"
        : "+v"(v));
    return v;
}
// the wave part of a row's maximum (one act group per row); the step across waves goes through the site's own LDS scratch
__device__ __forceinline__ float lut_wave_max(float mx) {
    mx = q_row_allmax(mx);
    return q_xor_max_f(mx);
}
// scales and t_scales of an act group from its abs-max: the two IEEE divisions, through div127 / rcp_exact (tmac_fastdiv.h) or, FDIV, as
// __fdiv_rn -- the same bits; k_gemv_quad's unified-scale path and k_preprocess_pairs_row keep the instructions they always had.
template <bool FDIV = false>
__device__ __forceinline__ void lut_scale(float mx, float& scales, float& t_scales) {
    if constexpr (FDIV) {
        scales = __fdiv_rn(mx, 127.0f);
        t_scales = (scales != 0.0f) ? __fdiv_rn(1.0f, scales) : 0.0f;
    } else {
        scales = div127(mx);
        t_scales = (scales != 0.0f) ? rcp_exact(scales) : 0.0f;
    }
}
// an act group of 64 activations = 8 lanes: its scale, in every lane of it
__device__ __forceinline__ void lut_group_scale(float x0, float x1, float x2, float x3, float x4, float x5, float x6, float x7,
                                                float& scales, float& t_scales) {
    lut_scale(q_half_allmax(lut_absmax8(x0, x1, x2, x3, x4, x5, x6, x7)), scales, t_scales);
}

// ---- tables ----------------------------------------------------------------------------------------------------------------
// One LUT table from its 4 activations: the 8 distinct magnitudes ((x0 +- x1) +- x2) +- x3 in the
// reference's association order, two per v_pk_add_f32; q = rne(L * t_scales) through the 1.5*2^23 magic add (|L * t_scales|
// <= 127 for finite input, so the sum's ulp is 1 and its low byte is q in two's complement; + 128 in the magic gives the
// biased byte).  Half table j = 0..7 holds {-L15, L1, -L13, L3, -L11, L5, -L9, L7}: negated entries as magic - product.
// Returns the dwords [j0 j1 j2 j3], [j4 j5 j6 j7] and L15 (its negation is the table's LUT[0], summed into lut_biases).
template <bool SIGNED>
__device__ __forceinline__ void q_table8(float x0, float x1, float x2, float x3, float t_scales, uint32_t& lo, uint32_t& hi, float& L15) {
    const qv2f x01 = {x0, x1}, x23 = {x2, x3};
    qv2f apm, l2m, l2p, L31, L119, L75, L1513;
    asm("v_pk_add_f32 %0, %1, %1 op_sel:[0,1] op_sel_hi:[0,1] neg_hi:[0,1]" : "=v"(apm) : "v"(x01));                      // {x0+x1, x0-x1}
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[1,0] neg_lo:[0,1] neg_hi:[0,1]" : "=v"(l2m) : "v"(apm), "v"(x23)); // {a_p-x2, a_m-x2}
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[1,0]" : "=v"(l2p) : "v"(apm), "v"(x23));                          // {a_p+x2, a_m+x2}
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,1] neg_lo:[0,1] neg_hi:[0,1]" : "=v"(L31) : "v"(l2m), "v"(x23)); // {L3, L1}
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,1]" : "=v"(L119) : "v"(l2m), "v"(x23));                         // {L11, L9}
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,1] neg_lo:[0,1] neg_hi:[0,1]" : "=v"(L75) : "v"(l2p), "v"(x23)); // {L7, L5}
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,1]" : "=v"(L1513) : "v"(l2p), "v"(x23));                        // {L15, L13}
    L15 = L1513.x;
    const qv2f tt = {t_scales, t_scales};
    const qv2f mg = {SIGNED ? 12582912.0f : 12583040.0f, 0.0f};
    qv2f za, zb, zc, zd;
    asm("v_pk_mul_f32 %0, %1, %2" : "=v"(za) : "v"(L31), "v"(tt));
    asm("v_pk_mul_f32 %0, %1, %2" : "=v"(zb) : "v"(L75), "v"(tt));
    asm("v_pk_mul_f32 %0, %1, %2" : "=v"(zc) : "v"(L119), "v"(tt));
    asm("v_pk_mul_f32 %0, %1, %2" : "=v"(zd) : "v"(L1513), "v"(tt));
    asm("v_pk_add_f32 %0, %1, %2 op_sel_hi:[1,0]" : "=v"(za) : "v"(za), "v"(mg));                                  // j = 3 | 1
    asm("v_pk_add_f32 %0, %1, %2 op_sel_hi:[1,0]" : "=v"(zb) : "v"(zb), "v"(mg));                                  // j = 7 | 5
    asm("v_pk_add_f32 %0, %1, %2 op_sel_hi:[1,0] neg_lo:[1,0] neg_hi:[1,0]" : "=v"(zc) : "v"(zc), "v"(mg));        // j = 4 | 6
    asm("v_pk_add_f32 %0, %1, %2 op_sel_hi:[1,0] neg_lo:[1,0] neg_hi:[1,0]" : "=v"(zd) : "v"(zd), "v"(mg));        // j = 0 | 2
    lo = __builtin_amdgcn_perm(__float_as_uint(za.y), __float_as_uint(zd.x), 0x0c0c0400u) |
         __builtin_amdgcn_perm(__float_as_uint(za.x), __float_as_uint(zd.y), 0x04000c0cu);
    hi = __builtin_amdgcn_perm(__float_as_uint(zb.y), __float_as_uint(zc.x), 0x0c0c0400u) |
         __builtin_amdgcn_perm(__float_as_uint(zb.x), __float_as_uint(zc.y), 0x04000c0cu);
}
// The two tables of a pair: {lo, hi} of table 2p | {lo, hi} of table 2p + 1, signed bytes (SIGNED: what the MFMA forms look up) or
// biased by 128; La, Lb = their L15.  As four words, or as the uint4 the images hold.
template <bool SIGNED>
__device__ __forceinline__ void lut_tables2_words(float x0, float x1, float x2, float x3, float x4, float x5, float x6, float x7,
                                                  float t_scales, uint32_t& lo0, uint32_t& hi0, uint32_t& lo1, uint32_t& hi1, float& La, float& Lb) {
    q_table8<SIGNED>(x0, x1, x2, x3, t_scales, lo0, hi0, La);
    q_table8<SIGNED>(x4, x5, x6, x7, t_scales, lo1, hi1, Lb);
}
template <bool SIGNED>
__device__ __forceinline__ uint4 lut_tables2(float x0, float x1, float x2, float x3, float x4, float x5, float x6, float x7,
                                             float t_scales, float& La, float& Lb) {
    uint32_t lo0, hi0, lo1, hi1;
    lut_tables2_words<SIGNED>(x0, x1, x2, x3, x4, x5, x6, x7, t_scales, lo0, hi0, lo1, hi1, La, Lb);
    return make_uint4(lo0, hi0, lo1, hi1);
}

// ---- lut_biases ------------------------------------------------------------------------------------------------------------
// LUT[0] of a table straight from its activations: -(((x0+x1)+x2)+x3), the adds q_table8 performs for L15
__device__ __forceinline__ float lut_lut0(float x0, float x1, float x2, float x3) { return -__fadd_rn(__fadd_rn(__fadd_rn(x0, x1), x2), x3); }
// The lane's two LUT[0] folded over the 4 lanes of a chunk; the chunk sum is va + vb (left to the caller: some sites add under a branch)
__device__ __forceinline__ void lut_chunk_fold(float& va, float& vb) {
    va = __fadd_rn(va, dpp_f<0x4E>(va));      // lane ^ 2: v0+v4 | v2+v6
    vb = __fadd_rn(vb, dpp_f<0x4E>(vb));      //           v1+v5 | v3+v7
    va = __fadd_rn(va, dpp_f<0xB1>(va));      // lane ^ 1: (v0+v4)+(v2+v6)
    vb = __fadd_rn(vb, dpp_f<0xB1>(vb));      //           (v1+v5)+(v3+v7)
}
// chunk sum from the L15 of the lane's two tables, in all 4 lanes of the chunk
__device__ __forceinline__ float lut_chunk_sum(float La, float Lb) {
    float va = -La, vb = -Lb;
    lut_chunk_fold(va, vb);
    return __fadd_rn(va, vb);
}
// Act group of two chunks (8 lanes): c1 = the second chunk's sum as the first chunk's lanes see it (row_shl:4; every lane of the act
// group executes it), then the group's bias in lane p & 7 == 0.  Two steps, so that a site keeps the adds inside its store branch.
__device__ __forceinline__ float lut_group_partner(float v) { return dpp_f<0x104>(v); }
__device__ __forceinline__ float lut_group_bias(float v, float c1) { return __fadd_rn(__fadd_rn(0.0f, v), c1); }

// One act group per row, pass 1, pair p: the lane's running abs-max and the chunk's sum (from x alone) to cs[p >> 2]
__device__ __forceinline__ void lut_row_pass1(float x0, float x1, float x2, float x3, float x4, float x5, float x6, float x7,
                                              int p, float& mx, float* cs) {
    mx = fmaxf(mx, lut_abssum4(x0, x1, x2, x3));
    mx = fmaxf(mx, lut_abssum4(x4, x5, x6, x7));
    float va = lut_lut0(x0, x1, x2, x3), vb = lut_lut0(x4, x5, x6, x7);
    lut_chunk_fold(va, vb);
    if ((p & 3) == 0) cs[p >> 2] = __fadd_rn(va, vb);
}

// ---- the workspace's other two layouts of a pair (t = lut_tables2<false>: biased bytes) --------------------------------------
// 16-table-segment half tables for k_gemv_lo -- tables 2p, 2p+1 are one uint4 of segment p >> 3 -- and the reference's int8 [K/4][16]:
// entries 0..7 signed, 8..15 = -entry(15 - j) (lut_ctor.cc:152-155); on biased bytes U in [1, 255] the bytewise negation 256 - U is one
// word subtraction without borrows
__device__ __forceinline__ void lut_store_ref_dev(const uint4 t, int K, int n, int p, uint4* __restrict__ qlut_ref,
                                                  uint2* __restrict__ qlut_dev, size_t qdev_u4_per_row) {
    const int seg = p >> 3, j8 = p & 7;
    *reinterpret_cast<uint4*>(qlut_dev + ((size_t)n * qdev_u4_per_row + qlut_dev_u4_index(seg, j8)) * 2) = t;
    const uint32_t sg = 0x80808080u, rev = 0x00010203u;
    const uint32_t n0l = __builtin_amdgcn_perm(0u, 0x01010100u - t.x, rev), n0h = __builtin_amdgcn_perm(0u, 0x01010100u - t.y, rev);
    const uint32_t n1l = __builtin_amdgcn_perm(0u, 0x01010100u - t.z, rev), n1h = __builtin_amdgcn_perm(0u, 0x01010100u - t.w, rev);
    uint4* r = qlut_ref + ((size_t)n * (K / 4) + 2 * (size_t)p);
    r[0] = make_uint4(t.x ^ sg, t.y ^ sg, n0h ^ sg, n0l ^ sg);
    r[1] = make_uint4(t.z ^ sg, t.w ^ sg, n1h ^ sg, n1l ^ sg);
}

}  // namespace tmac
