// tmac_experts_gemm.hip -- the grouped GEMM of a mixture-of-experts layer for N > 1 tokens, between k_experts_route and k_experts_combine
// (tmac_experts_rows.hip), and the LUT build that feeds it.  DESIGN.md 4.18.
//
// k_lut_image_pos: k_lut_image's build (tmac_gemm2.hip) in POSITION order -- image row p is the build of the activation row of position p:
// row src[p] / row_div of token-major activations x [N][K] (gate / up: row_div = S), or row p of position-major x [P][K] (down).  Where
// src[p] < 0 (padding, unused tiles) nothing is read from x and the row is zeros.  The gather sits here, in a latency-bound build at 2 bytes
// per activation, not in the GEMM's hot loop.
//
// k_gemm_experts<BITS, ZP, SCF16>: k_gemm_planes' arithmetic -- bit-planes merged in the A operand through the joint-index operand-row
// table in LDS, v_mfma_i32_32x32x32_i8 on a 64 rows x 64 positions wave tile, the zero-point term as v_mfma_f32_32x32x2_f32, one fp32 chain
// per output and act group -- restated here (a shared header with tmac_gemm2.hip is a follow-up), with a split of its own:
//   workgroup  four waves = ONE position tile t (blockIdx.y) x FOUR adjacent 64-row tiles of one bank (blockIdx.x); wave w owns row tile w.
//   K          every wave walks the whole K: no K split, no reduction through LDS, one barrier (behind the operand-row table).  The four
//              waves ask for the same B pieces (8 KB per step) at about the same time, so a CU fetches a step's 64 distinct lines once per
//              four wave-steps; each piece still goes global -> registers per wave, a scalar offset per act group, waits counted.
//   selection  the workgroup reads tile_expert[t] once, wave-uniform; a value outside [0, E) -- one unsigned compare -- ends it before any
//              other load.  Otherwise the bank's 16-byte ExpertEntry gives the weight and scale buffer resources.  Wave-uniform loads only.
//   LDS        64 KB of operand rows shared by the workgroup + 1 KB of weight scales / zeros per wave = 68 KB: two workgroups per CU.
//   stores     C[b][P][Mw] straight from the accumulators (a lane holds 4 x 4 consecutive rows of one position per 32 x 32 tile): a live
//              position its row, a padding position of a live tile +0.0, the rows of an unused tile nothing.
// An output is one wave's chain in plain K order: its bits depend on its (expert, activation row) alone.
// The unit is compiled without packed-fp32 instructions: the LUT build takes q_table8_single (tmac_lut_build.h), q_table8
// in single fp32 operations, and the fp32 chains are plain fmas.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>

#include "tmac_quad_core.h"
#include "tmac_lut_build.h"
#include "tmac_kernels.h"
#include "tmac_select.h"

#ifndef TMAC_EXPERTS_GEMM_BITS
#error "compile with -DTMAC_EXPERTS_GEMM_BITS=1..4 (one translation unit per weight width)"
#endif

namespace tmac {

typedef int e4i_t __attribute__((ext_vector_type(4)));
typedef int e16i_t __attribute__((ext_vector_type(16)));
typedef float e4f_t __attribute__((ext_vector_type(4)));
typedef float e16f_t __attribute__((ext_vector_type(16)));

#if TMAC_EXPERTS_GEMM_BITS == 1      // the LUT build has no width: it lives in the first unit
template <bool F16>
__global__ __launch_bounds__(256) void k_lut_image_pos(const void* __restrict__ x, const int32_t* __restrict__ src, int row_div, int x_rows,
                                                       uint4* __restrict__ bimg, float* __restrict__ colv, int K, int P) {
    const int kk = blockIdx.y;
    const int n = blockIdx.x * 32 + (threadIdx.x >> 3), p = threadIdx.x & 7;      // position n < P by the grid
    const int f = src[n];
    const uint32_t row = row_div ? (uint32_t)(f < 0 ? -1 : f / row_div) : (uint32_t)n;
    const bool live = f >= 0 && row < (uint32_t)x_rows;                          // the 8 lanes of an act group share n: uniform over them
    float v8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (live) lut_ld8(x, F16, (size_t)row * K + kk * 64, p, v8);
    float scales, t_scales, La, Lb;
    lut_group_scale(LUT_X8(v8), scales, t_scales);
    uint4 t;
    q_table8_single<true>(v8[0], v8[1], v8[2], v8[3], t_scales, t.x, t.y, La);
    q_table8_single<true>(v8[4], v8[5], v8[6], v8[7], t_scales, t.z, t.w, Lb);
    if (!live) t = make_uint4(0u, 0u, 0u, 0u);
    bimg[(((size_t)kk * (P >> 6) + (n >> 6)) * 8 + p) * 64 + (n & 63)] = t;
    int h = 0;
    const uint32_t d[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
    for (int i = 0; i < 4; ++i)
        h += (int)(int8_t)(d[i] & 0xff) + (int)(int8_t)((d[i] >> 8) & 0xff) + (int)(int8_t)((d[i] >> 16) & 0xff) + ((int)d[i] >> 24);
    h += (int)dpp_u<0xB1>((uint32_t)h);
    h += (int)dpp_u<0x4E>((uint32_t)h);
    h += (int)dpp_u<0x104>((uint32_t)h);
    const float v = lut_chunk_sum(La, Lb);
    const float c1 = lut_group_partner(v);
    if (p == 0) {
        const float lb = lut_group_bias(v, c1);
        reinterpret_cast<float4*>(colv)[(size_t)kk * P + n] =
            live ? make_float4(__fmul_rn(0.5f, scales), __fmul_rn(0.5f, lb), (float)h, lb) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

hipError_t launch_lut_image_pos(const void* x, int act_f16, const int32_t* src, int row_div, int x_rows, void* bimg, float* colv, int K, int P,
                                hipStream_t st) {
    if (!x || !src || !bimg || !colv || K < 64 || K % 64 != 0 || P < 64 || P % 64 != 0 || row_div < 0 || x_rows < 1) return hipErrorInvalidValue;
    if (row_div == 0 && x_rows != P) return hipErrorInvalidValue;                // position-major: one row per position
    const dim3 g(P / 32, K / 64), b(256);
    if (act_f16) hipLaunchKernelGGL(k_lut_image_pos<true>, g, b, 0, st, x, src, row_div, x_rows, (uint4*)bimg, colv, K, P);
    else hipLaunchKernelGGL(k_lut_image_pos<false>, g, b, 0, st, x, src, row_div, x_rows, (uint4*)bimg, colv, K, P);
    return hipGetLastError();
}
#endif

// a pointer every lane holds the same value of, as the scalar the buffer resource wants
__device__ __forceinline__ const void* uni_ptr(const void* p) {
    const uint64_t v = (uint64_t)(uintptr_t)p;
    return (const void*)(uintptr_t)(((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) |
                                    (uint32_t)__builtin_amdgcn_readfirstlane((int)v));
}

constexpr int EG_PAT_BYTES = 256 * 32 * 8, EG_SC_WAVE = 2 * 512;
static_assert(EG_PAT_BYTES + EXPERTS_GEMM_NWV * EG_SC_WAVE == EXPERTS_GEMM_LDS_BYTES, "the planner's LDS bytes are the kernel's");

template <int BITS, bool ZP, bool SCF16>
__global__ __launch_bounds__(64 * EXPERTS_GEMM_NWV, 2) void k_gemm_experts(ExpertsGemmArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char plds[];
    constexpr int NJ = BITS;                   // uint4 per unit and row quad in the QUAD layout
    constexpr bool ODD = (BITS & 1) != 0;      // 1- / 3-bit weights: 16-byte table entries, a lane holds one whole unit per tile row
    constexpr int WPU = ODD ? BITS : BITS / 2; // uint4 of weights per lane, tile row and [even widths: unit | odd: act group]
    constexpr int WUN = ODD ? 1 : 2;
    constexpr int BIASB = BITS == 4 ? 15 : BITS == 3 ? 7 : 0;   // what the biased operand bytes add per half-table entry
    const int tid = threadIdx.x, w = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int kb = lane >> 5, j = lane & 31;

    // ---- device-side selection: the tile's expert, then the bank's entry.  Wave-uniform loads; no address is formed from a value
    //      outside [0, E)
    const int t = blockIdx.y;
    int bx = blockIdx.x;
    const int bi = (a.nbanks > 1 && bx >= a.b[0].wg_end) ? 1 : 0;
    if (bi) bx -= a.b[0].wg_end;
    const ExpertsGemmBank bk = bi ? a.b[1] : a.b[0];
    const uint32_t e = (uint32_t)__builtin_amdgcn_readfirstlane(a.tile_expert[t]);
    if (e >= (uint32_t)bk.E) return;           // an unused tile: its rows are not written
    const ExpertEntry ent = bk.tab[e];
    const void* const W = uni_ptr(ent.W);
    const void* const SC = uni_ptr(ent.SC);

    const int K = a.s.K, Mw = bk.Mw, G = K / 64, nu = K / 32, nst = (nu + 63) >> 6, nq = Mw >> 2;
    const int row0 = (bx * EXPERTS_GEMM_NWV + w) * 64, n0 = t * 64;
    const int apg_sh = a.apg_shift, apg_m = (1 << apg_sh) - 1, nsg = G >> apg_sh;      // act groups per weight group: 1 << apg_sh
    const bool work = row0 < Mw;               // (a wave past the bank's rows still builds its part of the operand rows)

    const uint32_t psel = 0x0c0c0000u | ((4u + (lane & 3)) << 8);
    const uint32_t copyoff = ODD ? (uint32_t)(lane & 15) * 16u : (uint32_t)j * 8u;
    const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(W), (short)0, 0x7fffffff, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_b = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint4*>(a.bimg), (short)0, 0x7fffffff, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_c = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.colv), (short)0, 0x7fffffff, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_s = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(SC), (short)0, 0x7fffffff, 0x00020000);
    int wvoff[2];                              // byte offset of (row quad of this lane in tile row rt, uint4 kb [W2] / 2 kb [W4]) in the weights
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
        const int quad = max(min((row0 >> 2) + rt * 8 + (j >> 2), nq - 1), 0);
        wvoff[rt] = ODD ? (quad * nst * NJ * 64 + kb) * 16 : ((quad * nst * NJ + (BITS == 2 ? kb : 2 * kb)) * 64) * 16;
    }
    // chunk-major position image: the chunk of (act group, position tile) is 8 KB in one piece, the column values one float4 per position
    const int cvoff = (n0 + j) * 16, chunk_stride = (a.P >> 6) * 8192, col_stride = a.P * 16;
    constexpr int SC_ESZ = SCF16 ? 2 : 4, SC_PER = ZP ? 2 : 1;
    const int scvoff = (max(min((row0 >> 2) + (lane >> 2), nq - 1), 0) * nsg * 4 + (lane & 3)) * SC_PER * SC_ESZ;   // quad_scale_index, group 0
    const uint32_t sc_wave = EG_PAT_BYTES + w * EG_SC_WAVE;

    uint4 wv[WUN][2][WPU];
    uint32_t st_sc = 0u, st_zr = 0u, st0_sc = 0u, st0_zr = 0u;    // raw scale / zero of row (row0 + lane) of the NEXT weight group, one slot
    float lbs[2] = {0.f, 0.f};
    float za[2] = {0.f, 0.f}, zb[2] = {0.f, 0.f};
    e4i_t bv[2][4];                            // B operands: [position half][32-deep step], loaded a step ahead, in place
    const int bdvoff = ((ODD ? kb * 4 : 2 * kb) * 64 + j) * 16;
    auto load_b = [&](int kk, int nt) {
        const int so = kk * chunk_stride + t * 8192;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const int c = ODD ? (ks * 64 + nt * 32) * 16 : ((ks & 1) * 64 + nt * 32) * 16;
            const u32x4q v = __builtin_amdgcn_raw_buffer_load_b128(rs_b, bdvoff + c, ODD ? so : so + (ks >> 1) * 4096, 0);
            bv[nt][ks] = (e4i_t){(int)v[0], (int)v[1], (int)v[2], (int)v[3]};
        }
    };
    auto load_weights = [&](int kk, int rt) {
        const int u0 = 2 * kk, so = ((u0 >> 6) * NJ * 64 + (u0 & 63)) * 16;
#pragma unroll
        for (int ul = 0; ul < WUN; ++ul) {
#pragma unroll
            for (int q = 0; q < WPU; ++q) {
                const u32x4q v = __builtin_amdgcn_raw_buffer_load_b128(rs_w, wvoff[rt] + ul * 16 + q * 1024, so, 0);
                wv[ul][rt][q] = make_uint4(v[0], v[1], v[2], v[3]);
            }
        }
    };
    // (the dynamic LDS block starts at LDS address 0 -- the kernel has no static LDS -- so the perm's result IS the address)
    typedef unsigned int e2u_t __attribute__((ext_vector_type(2)));
    typedef unsigned int e4u_t __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(3))) const e2u_t* lds_u2_ptr;
    typedef __attribute__((address_space(3))) const e4u_t* lds_u4_ptr;
    auto pat_row = [&](uint32_t d) -> uint2 {
        const e2u_t v = *(lds_u2_ptr)(uintptr_t)__builtin_amdgcn_perm(d, copyoff, psel);
        return make_uint2(v.x, v.y);
    };
    auto pat_row2 = [&](uint32_t d) -> uint4 {  // odd widths: the operand rows of the byte's two nibbles
        const e4u_t v = *(lds_u4_ptr)(uintptr_t)__builtin_amdgcn_perm(d, copyoff, psel);
        return make_uint4(v.x, v.y, v.z, v.w);
    };
    auto load_staged = [&](int g) {            // scale / zero of row (row0 + lane), weight group g -> registers, raw
        const int so = g * 4 * SC_PER * SC_ESZ;
        if constexpr (SCF16) {
            if (ZP) st_sc = __builtin_amdgcn_raw_buffer_load_b32(rs_s, scvoff, so, 0);
            else st_sc = __builtin_amdgcn_raw_buffer_load_b16(rs_s, scvoff, so, 0);
        } else {
            st_sc = __builtin_amdgcn_raw_buffer_load_b32(rs_s, scvoff, so, 0);
            if (ZP) st_zr = __builtin_amdgcn_raw_buffer_load_b32(rs_s, scvoff + 4, so, 0);
        }
    };
    auto st_val = [&](uint32_t raw) -> float {
        if constexpr (SCF16) return __half2float(__ushort_as_half((unsigned short)raw));
        else return __uint_as_float(raw);
    };
    auto write_staged = [&](int g) {           // the staged values are group g's; LDS buffer g & 1
        float* p = reinterpret_cast<float*>(plds + sc_wave + (g & 1) * 512);
        if constexpr (SCF16 && ZP) {
            p[lane] = st_val(st_sc & 0xffffu);
            p[64 + lane] = st_val(st_sc >> 16);
        } else {
            p[lane] = st_val(st_sc);
            if (ZP) p[64 + lane] = st_val(st_zr);
        }
    };
    // accumulator rows of this lane in tile row rt: 8 q4 + 4 kb + (0..3), q4 = 0..3
    auto read_rows = [&](int buf, int rt, float (&dst)[16]) {
        const unsigned char* p = plds + sc_wave + buf * 512;
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
            const e4f_t v = *reinterpret_cast<const e4f_t*>(p + (32 * rt + 8 * q4 + 4 * kb) * 4);
            dst[4 * q4] = v.x; dst[4 * q4 + 1] = v.y; dst[4 * q4 + 2] = v.z; dst[4 * q4 + 3] = v.w;
        }
    };
    u32x4q cn[2];                              // column values of the NEXT act group, per position half
    auto load_cols = [&](int kk) {
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) cn[nt] = __builtin_amdgcn_raw_buffer_load_b128(rs_c, cvoff + nt * 512, kk * col_stride, 0);
    };
    if (work) {                                // everything the first step needs is in flight while the operand rows are built,
        load_staged(0);                        // in the order a step issues the loads of its successor
        st0_sc = st_sc; st0_zr = st_zr;
        load_staged(1 < nsg ? 1 : 0);
        load_cols(0);
        load_weights(0, 0);
        load_weights(0, 1);
        load_b(0, 0); load_b(0, 1);
    }

    // ---- joint-index operand rows: entry b = (i1 << 4) | i0, byte e = s(i0) [e == i0 & 7] + 2 s(i1) [e == i1 & 7] (+ 3 for W4); one
    //      thread per entry, 32 copies of 8 bytes / 16 of 16
    {
        const int b = tid & 255, i0 = b & 15, i1 = b >> 4;
        uint32_t lo = 0, hi = 0, lo1 = 0, hi1 = 0;
#pragma unroll
        for (int en = 0; en < 8; ++en) {
            if (ODD) {                         // one plane per nibble: +-1 (W3: + 1), low nibble's row | high nibble's row
                const int v0 = (BITS == 3 ? 1 : 0) + (en == (i0 & 7) ? ((i0 & 8) ? -1 : 1) : 0);
                const int v1 = (BITS == 3 ? 1 : 0) + (en == (i1 & 7) ? ((i1 & 8) ? -1 : 1) : 0);
                const uint32_t b0 = (uint32_t)(v0 & 0xff) << (8 * (en & 3)), b1 = (uint32_t)(v1 & 0xff) << (8 * (en & 3));
                if (en < 4) { lo |= b0; lo1 |= b1; } else { hi |= b0; hi1 |= b1; }
            } else {
                int v = (BITS == 4) ? 3 : 0;
                if (en == (i0 & 7)) v += (i0 & 8) ? -1 : 1;
                if (en == (i1 & 7)) v += (i1 & 8) ? -2 : 2;
                const uint32_t by8 = (uint32_t)(v & 0xff) << (8 * (en & 3));
                if (en < 4) lo |= by8; else hi |= by8;
            }
        }
        if (!ODD) { lo1 = lo; hi1 = hi; }
        uint4* pt = reinterpret_cast<uint4*>(plds) + b * 16;
#pragma unroll
        for (int c = 0; c < 16; ++c) pt[(c + b) & 15] = make_uint4(lo, hi, lo1, hi1);
    }
    __syncthreads();                           // the kernel's one barrier
    if (!work) return;

    e16f_t facc[2][2];                         // whole register tuples: the zero-point MFMA takes and returns them in place
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) facc[rt][nt][r] = 0.f;
    {
        const uint32_t k_sc = st_sc, k_zr = st_zr;
        st_sc = st0_sc; st_zr = st0_zr;
        write_staged(0);
        st_sc = k_sc; st_zr = k_zr;
    }
    // W1 / W2: accumulators start from the bits of 3.0f, so that int -> float is one subtraction (3 + comb * 2^-22 exactly, |comb| < 2^19)
    constexpr bool MAGIC = BITS <= 2;
    constexpr int CI = MAGIC ? 0x40400000 : 0;
    e16i_t cinit = {CI, CI, CI, CI, CI, CI, CI, CI, CI, CI, CI, CI, CI, CI, CI, CI};
    if (MAGIC) asm volatile("" : "+v"(cinit));
    auto build_av = [&](int rt, e4i_t (&av)[4]) {       // A operands of tile row rt: the joint plane index of (row, table) selects the operand row
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            if constexpr (BITS == 1) {             // dword ks of the unit = tables 2 ks, 2 ks + 1
                const uint4 q = wv[0][rt][0];
                const uint4 g = pat_row2(ks == 0 ? q.x : ks == 1 ? q.y : ks == 2 ? q.z : q.w);
                av[ks] = (e4i_t){(int)g.x, (int)g.y, (int)g.z, (int)g.w};
            } else if constexpr (BITS == 3) {      // dwords 3 ks .. 3 ks + 2 of the unit's twelve
                const uint32_t dw[12] = {wv[0][rt][0].x, wv[0][rt][0].y, wv[0][rt][0].z, wv[0][rt][0].w, wv[0][rt][1].x, wv[0][rt][1].y,
                                         wv[0][rt][1].z, wv[0][rt][1].w, wv[0][rt][2].x, wv[0][rt][2].y, wv[0][rt][2].z, wv[0][rt][2].w};
                const uint4 g0 = pat_row2(dw[3 * ks]), g1 = pat_row2(dw[3 * ks + 1]), g2 = pat_row2(dw[3 * ks + 2]);
                av[ks] = (e4i_t){(int)(g0.x + (g0.z << 1) + (g1.x << 2)), (int)(g0.y + (g0.w << 1) + (g1.y << 2)),
                                 (int)(g1.z + (g2.x << 1) + (g2.z << 2)), (int)(g1.w + (g2.y << 1) + (g2.w << 2))};
            } else if constexpr (BITS == 2) {
                const uint4 q = wv[ks >> 1][rt][0];
                const uint2 t0 = pat_row((ks & 1) ? q.z : q.x), t1 = pat_row((ks & 1) ? q.w : q.y);
                av[ks] = (e4i_t){(int)t0.x, (int)t0.y, (int)t1.x, (int)t1.y};
            } else {
                const uint4 q = wv[ks >> 1][rt][ks & 1];
                const uint2 a0 = pat_row(q.x), a1 = pat_row(q.y), b0 = pat_row(q.z), b1 = pat_row(q.w);
                av[ks] = (e4i_t){(int)(a0.x + (a1.x << 2)), (int)(a0.y + (a1.y << 2)), (int)(b0.x + (b1.x << 2)), (int)(b0.y + (b1.y << 2))};
            }
        }
    };
    // One act group (64 activations = four 32-deep MFMA steps) per iteration, k_gemm_planes' order of phases: the operands of tile row 1
    // are fetched while the MFMAs of tile row 0 run, the fp32 chain of a tile runs under the MFMAs of the next; the loads of the next act
    // group are unconditional (the last step fetches its own again) so that the step is one block and every wait is counted.
    for (int kk = 0; kk < G; ++kk) {
        const int g = kk >> apg_sh;
        const bool glast = (kk & apg_m) == apg_m;          // last act group of its weight group
        const bool more = glast && g + 1 < nsg;
        const int cbuf = g & 1;
        if (more) write_staged(g + 1);
        e4i_t av0[4], av1[4];
        float sc[16];                          // row scales of the tile row in work: tile row 1's replace tile row 0's behind their last chain
        build_av(0, av0);
        read_rows(cbuf, 0, sc);
        // column values of the act group: v = x * H + hlbx with x = comb * 2^-22, H = (ls / 2) * 2^22, hlbx = lb / 2
        // [- BIASB * (entry sum) * (ls / 2) for the biased operand bytes of W3 / W4]
        float H[2], hlbx[2], lb[2];
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            const float hls = __uint_as_float(cn[nt][0]);
            lb[nt] = __uint_as_float(cn[nt][3]);
            H[nt] = MAGIC ? __fmul_rn(hls, 4194304.0f) : hls;
            hlbx[nt] = __uint_as_float(cn[nt][1]);
            if (BIASB) hlbx[nt] = __fmaf_rn(-__fmul_rn((float)BIASB, __uint_as_float(cn[nt][2])), hls, hlbx[nt]);
        }
        const int kn = kk + 1 < G ? kk + 1 : kk;
        { const int gs2 = ((kn >> apg_sh) + 1 < nsg) ? (kn >> apg_sh) + 1 : nsg - 1; load_staged(gs2); }
        load_cols(kn); load_weights(kn, 0);
        __builtin_amdgcn_sched_barrier(0);

        auto chain = [&](const e4i_t (&av)[4], int nt, e16i_t& c) {      // one 32 x 32 tile of the act group: four dependent MFMAs
            c = __builtin_amdgcn_mfma_i32_32x32x32_i8(av[0], bv[nt][0], cinit, 0, 0, 0);
#pragma unroll
            for (int ks = 1; ks < 4; ++ks) c = __builtin_amdgcn_mfma_i32_32x32x32_i8(av[ks], bv[nt][ks], c, 0, 0, 0);
        };
        // C += ((comb / 2) ls + lb / 2) scale: three passes of independent instructions over the lane's 16 values
        auto epilogue = [&](int rt, int nt, const e16i_t& c, const float (&sc)[16]) {
            float x[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) x[r] = MAGIC ? __fsub_rn(__int_as_float(c[r]), 3.0f) : (float)c[r];
#pragma unroll
            for (int r = 0; r < 16; ++r) x[r] = __fmaf_rn(x[r], H[nt], hlbx[nt]);
#pragma unroll
            for (int r = 0; r < 16; ++r) facc[rt][nt][r] = __fmaf_rn(x[r], sc[r], facc[rt][nt][r]);
        };
        // the zero-point term of a weight group, zero[o] * (sum of its lut_biases)[n], is a rank-1 update of the tile: two weight groups
        // make one v_mfma_f32_32x32x2_f32 per 32 x 32 tile (k = the group's parity; lane (kb, j) holds row / column j of group kb)
        auto zero_stage = [&]() {
            const float* zp = reinterpret_cast<const float*>(plds + sc_wave + cbuf * 512 + 256);
            const bool mine = kb == cbuf;
#pragma unroll
            for (int rt = 0; rt < 2; ++rt) {
                const float z = zp[32 * rt + j];
                za[rt] = mine ? z : (cbuf ? za[rt] : 0.f);
            }
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                const float l = __fadd_rn(lbs[nt], lb[nt]);
                zb[nt] = mine ? l : (cbuf ? zb[nt] : 0.f);
            }
        };
        auto zero_flush = [&]() {
#pragma unroll
            for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt)
                    facc[rt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(za[rt], zb[nt], facc[rt][nt], 0, 0, 0);
        };

        e16i_t ca, cb;
        chain(av0, 0, ca);
        chain(av0, 1, cb);
        __builtin_amdgcn_sched_barrier(0);
        build_av(1, av1);
        load_weights(kn, 1);
        __builtin_amdgcn_sched_barrier(0);
        epilogue(0, 0, ca, sc);
        __builtin_amdgcn_sched_barrier(0);
        chain(av1, 0, ca);
        load_b(kn, 0);                         // (position half 0's operands have been read by their last chain)
        __builtin_amdgcn_sched_barrier(0);
        epilogue(0, 1, cb, sc);
        read_rows(cbuf, 1, sc);
        __builtin_amdgcn_sched_barrier(0);
        chain(av1, 1, cb);
        load_b(kn, 1);
        __builtin_amdgcn_sched_barrier(0);
        epilogue(1, 0, ca, sc);
        __builtin_amdgcn_sched_barrier(0);
        epilogue(1, 1, cb, sc);
        if (ZP && glast) { zero_stage(); if (cbuf || g + 1 >= nsg) zero_flush(); }
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) lbs[nt] = glast ? 0.f : __fadd_rn(lbs[nt], lb[nt]);
    }

    // ---- store: lane (kb, j) holds rows 32 rt + 8 q4 + 4 kb + (0..3) of position n0 + 32 nt + j; a padding position gets +0.0
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        const int p = n0 + nt * 32 + j;
        const bool live = a.src[p] >= 0;
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                const int o = row0 + 32 * rt + 8 * q4 + 4 * kb;
                if (o >= Mw) continue;         // (Mw is a multiple of 4: a quartet is inside or outside)
                const e16f_t& f = facc[rt][nt];
                const e4f_t v = live ? (e4f_t){f[4 * q4], f[4 * q4 + 1], f[4 * q4 + 2], f[4 * q4 + 3]} : (e4f_t){0.f, 0.f, 0.f, 0.f};
                if (a.out_f16) {
                    const __half2 h0 = __floats2half2_rn(v.x, v.y), h1 = __floats2half2_rn(v.z, v.w);
                    *reinterpret_cast<uint2*>(reinterpret_cast<__half*>(bk.C) + (size_t)p * Mw + o) =
                        make_uint2(*reinterpret_cast<const uint32_t*>(&h0), *reinterpret_cast<const uint32_t*>(&h1));
                } else {
                    *reinterpret_cast<e4f_t*>(reinterpret_cast<float*>(bk.C) + (size_t)p * Mw + o) = v;
                }
            }
    }
}

template <int BITS>
hipError_t launch_gemm_experts_unit(const ExpertsGemmArgs& a, const ExpertsGemmPlan& p, hipStream_t st) {
    const dim3 g(p.gx, p.gy), b(64 * EXPERTS_GEMM_NWV);
    return sel_bool(a.s.zero_point != 0, [&](auto ZP) { return sel_bool(a.sc_f16 != 0, [&](auto SCF16) {
        static size_t allowed = 0;             // dynamic LDS above 64 KB is allowed per kernel, once
        return launch_lds_once(allowed, p.lds_bytes, k_gemm_experts<BITS, ZP, SCF16>, g, b, p.lds_bytes, st, a);
    }); });
}
template hipError_t launch_gemm_experts_unit<TMAC_EXPERTS_GEMM_BITS>(const ExpertsGemmArgs&, const ExpertsGemmPlan&, hipStream_t);

}  // namespace tmac
