// tmac_rows.hip -- k_gemv_rows: 2-8 activation rows per weight pass (N > 1 below the GEMM crossover), stand-alone launches.
//
// Work decomposition of k_gemv_quad: a WAVE owns a row quad, its 64 lanes hold the 64 units of a 64-unit step; persistent eight-wave
// workgroups walk their (quad, step) list, 1 / 2 / 4 waves per quad splitting the steps (combined through LDS in wave order).  The item is
// built from tmac_chain_core.h: CFrag / c_issue for the weight fragment (scales in the fragment), c_selectors and the lookups + MFMA adder +
// per-act-group fp32 chain of c_compute.  The one new idea: a fragment is loaded ONCE and the lookups run once per live activation row, each
// row with its own tables, LUT scales / biases and accumulator -- weights and weight scales are fetched once per row GROUP, not once per row.
//   R    row capacity of the workgroup (2, 4, 8): LDS holds R rows of exactly what k_gemv_quad holds for one; nr <= R rows are live,
//        rows r >= nr are skipped by a wave-uniform branch, never copied, never stored
//   blockIdx.y = row group: rows n_base + y * rows_per_group ... (the grouping is rows_plan's, a pure host function)
// The tables are COPIED from the workspace's half-table image exactly as k_gemv_quad does with LUTSRC == 0 (xor 0x80808080 for the MFMA
// adder, scales halved, zero tables between nu and the end of the last step): no LUT is built here, the tables are today's bit for bit.
// r_compute below is c_compute's non-IMG2 body with ONE difference: the weight scales arrive decoded and per act group, because a lane's two
// act groups of a step lie in two scale groups when gs = 64 (the plain c_issue / c_compute carry one scale group per lane and step; their G2
// instantiations carry both at compile time, this kernel decides at run time: the second one is fetched beside the fragment).  No waits between workgroups, no spins, no atomics.  DESIGN.md 4.9.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>

#include "tmac_core.h"
#include "tmac_kernels.h"
#include "tmac_chain_core.h"
#include "tmac_select.h"

namespace tmac {

template <int BITS>
struct RFrag {
    CFrag<BITS> c;
    uint32_t t0, t1;      // gs = 64 only: scale (, zero) of the lane's SECOND act group of the step (layout of c.s0, c.s1)
};

template <bool ZP, bool SCF16>
__device__ __forceinline__ void r_decode(uint32_t s0, uint32_t s1, float& sc, float& zr) {
    zr = 0.f;
    if (SCF16) {
        sc = __half2float(__ushort_as_half((unsigned short)(s0 & 0xffff)));
        if (ZP) zr = __half2float(__ushort_as_half((unsigned short)(s0 >> 16)));
    } else {
        sc = __uint_as_float(s0);
        if (ZP) zr = __uint_as_float(s1);
    }
}

// One 64-unit step of a row quad against ONE activation row's tables (c_compute, tmac_chain_core.h): per-group scales -> the two act
// groups of the lane's output row through the fp32 chain into cacc; unified scales -> exact int32 totals per plane into iacc.
template <int BITS, bool ZP, int SM>
__device__ __forceinline__ void r_compute(const CFrag<BITS>& f, const uint4* tab, int tstride, const float* l_ls, const float* l_lb, int ub,
                                          uint32_t lane16, uint32_t lk4, const CSel<BITS>& sel, uint32_t k3, float sc0, float zr0, float sc1,
                                          float zr1, float& cacc, int32_t (&iacc)[BITS], int32_t* tap_row, int G) {
    uint32_t tb[16];
#pragma unroll
    for (int j4 = 0; j4 < 4; ++j4) {
        // units past K read the zero tables: no contribution
        const uint4 v = *reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(tab + (j4 * tstride + ub)) + lane16);
        tb[4 * j4] = v.x; tb[4 * j4 + 1] = v.y; tb[4 * j4 + 2] = v.z; tb[4 * j4 + 3] = v.w;
    }
    constexpr int NACC = (SM == 0) ? 1 : BITS;
    qv4i_t c[NACC];
#pragma unroll
    for (int pl = 0; pl < NACC; ++pl) c[pl] = (qv4i_t){0, 0, 0, 0};
#pragma unroll
    for (int tp = 0; tp < 4; ++tp) {
#pragma unroll
        for (int pl = 0; pl < BITS; ++pl) {
            uint32_t pa, ma, pb, mb;
            const int qa = (2 * tp) * BITS + pl, qb = (2 * tp + 1) * BITS + pl;
            if (qa & 1) q_lookup4_pm<1>(f.wq[qa >> 3][(qa >> 1) & 3], tb[4 * tp], tb[4 * tp + 1], k3, pa, ma);
            else q_lookup4_pm<0>(f.wq[qa >> 3][(qa >> 1) & 3], tb[4 * tp], tb[4 * tp + 1], k3, pa, ma);
            if (qb & 1) q_lookup4_pm<1>(f.wq[qb >> 3][(qb >> 1) & 3], tb[4 * tp + 2], tb[4 * tp + 3], k3, pb, mb);
            else q_lookup4_pm<0>(f.wq[qb >> 3][(qb >> 1) & 3], tb[4 * tp + 2], tb[4 * tp + 3], k3, pb, mb);
            qv4i_t& cd = c[(SM == 0) ? 0 : pl];
            cd = __builtin_amdgcn_mfma_i32_16x16x64_i8((qv4i_t){(int)pa, (int)ma, (int)pb, (int)mb}, sel.p[pl], cd, 0, 0, 0);
        }
    }
    if constexpr (SM == 2) {
        // the MFMA results must have landed before a VALU instruction reads them: one wait behind the last MFMA of the step (see c_compute)
        if constexpr (BITS == 1) asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 3" : "+v"(c[0]));
        else if constexpr (BITS == 2) asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 3" : "+v"(c[0]), "+v"(c[1]));
        else if constexpr (BITS == 3) asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 3" : "+v"(c[0]), "+v"(c[1]), "+v"(c[2]));
        else asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 3" : "+v"(c[0]), "+v"(c[1]), "+v"(c[2]), "+v"(c[3]));
#pragma unroll
        for (int pl = 0; pl < BITS; ++pl) iacc[pl] += (c[pl].x + c[pl].y) + (c[pl].z + c[pl].w);
    } else {
        // act groups ub / 2 + lk4 / 4 + {0, 1}: ls / 2 and lb / 2 (groups past K hold zeros)
        const float2 hls2 = *reinterpret_cast<const float2*>(reinterpret_cast<const char*>(l_ls + (ub >> 1)) + lk4);
        const float2 hlb2 = *reinterpret_cast<const float2*>(reinterpret_cast<const char*>(l_lb + (ub >> 1)) + lk4);
#pragma unroll
        for (int gi = 0; gi < 2; ++gi) {
            const float hls = gi ? hls2.y : hls2.x, hlb = gi ? hlb2.y : hlb2.x;
            const float sc = gi ? sc1 : sc0, zr = gi ? zr1 : zr0;
            // sum_p alpha_p [(ps_p ls + [p = 0] lb) scale + [p = 0] zero 2 lb] = ((sum_p 2^p ps_p)(ls / 2) + lb / 2) scale + (2 zero)(lb / 2)
            const int32_t comb = (gi == 0) ? (c[0].x + c[0].y) : (c[0].z + c[0].w);
            if (tap_row) {
                const int kk = (ub >> 1) + (int)(lk4 >> 2) + gi;
                if (kk < G) tap_row[kk] = comb;
            }
            const float v = __fmaf_rn((float)comb, hls, hlb);
            float cc = __fmaf_rn(v, sc, cacc);
            if (ZP) cc = __fmaf_rn(__fadd_rn(zr, zr), hlb, cc);
            cacc = cc;
        }
    }
}

template <int BITS, bool ZP, bool SCF16, int SM, int R>
__global__ __launch_bounds__(ROWS_FT) void k_gemv_rows(RowsArgs a) {
    extern __shared__ uint4 lds[];
    constexpr int NWV = ROWS_NWV, FT = ROWS_FT;
    const int tid = threadIdx.x, w = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int n0 = a.n_base + (int)blockIdx.y * a.rows_per_group;
    const int nr = min(R, a.N - n0);                                  // live rows of this group (uniform)
    const int nu = a.nu, nst = a.nst, G = a.G;
    const int tstride = nst * 64 + 1;                                 // whole steps: units past K hold zero tables
    const int GP = nst * 32;                                          // act groups of the padded steps (>= G)
    const int row_u4 = 4 * tstride + GP / 2;                          // per row: [4][tstride] uint4 tables | ls / 2 [GP] | lb / 2 [GP]
    float* l_red = reinterpret_cast<float*>(lds + (size_t)R * row_u4);   // [2][R][NWV][4 rows][4]: partials of the waves of a quad
    const int wpq = a.wpq, IPI = NWV / wpq;
    const bool two_sg = SM == 0 && a.gs_shift < 2;                    // gs = 64: the lane's two act groups have a scale group each

    const int nmat = a.nmat;
    const int total_q = a.m[nmat - 1].nb_end;                         // cumulative QUAD counts
    struct MatCur { FusedMat m; int base, mi, end; };                 // (k_gemv_quad) end: first quad past this matrix
    auto seek = [&](MatCur& c, int gq) {
        while (gq >= c.end) { c.base = c.m.nb_end; ++c.mi; c.m = a.m[c.mi]; c.end = (c.mi + 1 < nmat) ? c.m.nb_end : 0x7fffffff; }
    };
    MatCur pc = {a.m[0], 0, 0, nmat > 1 ? a.m[0].nb_end : 0x7fffffff}, cc = pc;

    uint32_t lane16 = (uint32_t)lane * 16u;                           // the lane's 16 bytes of a table row / weight block
    asm volatile("" : "+v"(lane16));
    uint32_t lk4 = 4u * (uint32_t)(2 * (lane & 12) + 2 * (lane >> 4));   // the lane's two act groups inside a step's 32
    asm volatile("" : "+v"(lk4));

    // ---- 1. this wave's work: quads slot, slot + stride, ...; steps h, h + wpq, ... of each; first fragments issued BEFORE the table
    //         copy, so the weight stream overlaps it (the order k_gemv_quad measured as the one that matters) ------------------------
    const int slot0 = (int)blockIdx.x * IPI + w / wpq, h = w % wpq, stride = (int)gridDim.x * IPI;
    constexpr int RING = (BITS <= 2) ? 4 : 2;                         // weight fragments in flight per wave
    RFrag<BITS> f0, f1, f2, f3;
    int p_q = (h < nst) ? slot0 : total_q, p_st = h;                  // prefetch cursor
    constexpr int per = ZP ? 2 : 1, esz = SCF16 ? 2 : 4;
    auto issue = [&](RFrag<BITS>& f) {
        if (p_q < total_q) {
            seek(pc, p_q);
            const int lq = p_q - pc.base;
            const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint4*>(pc.m.W), (short)0, 0x7fffffff, 0x00020000);
            const TMAC_GLOBAL char* scq = (const TMAC_GLOBAL char*)pc.m.SC + (size_t)lq * (size_t)(a.nsg * 4 * per * esz);
            c_issue<BITS, ZP, SCF16, SM>(f.c, rs, lq * nst * (BITS * 1024), scq, a.nsg, a.gs_shift, nu, p_st, lane, lane16);
            uint32_t r0 = 0, r1 = 0;
            if (two_sg) {           // clamped, not predicated: groups past K meet zero tables and zero LUT scales
                const int c0 = 4 * (lane & 12) + 4 * (lane >> 4) + 2;
                const uint32_t sg = min((uint32_t)p_st * (64u >> a.gs_shift) + (uint32_t)(c0 >> a.gs_shift), (uint32_t)a.nsg - 1u);
                const uint32_t boff = (sg * 4 + (lane & 3)) * (per * esz);
                if (SCF16) {
                    if (ZP) r0 = *reinterpret_cast<const TMAC_GLOBAL uint32_t*>(scq + boff);
                    else r0 = *reinterpret_cast<const TMAC_GLOBAL unsigned short*>(scq + boff);
                } else {
                    const TMAC_GLOBAL uint32_t* p32 = reinterpret_cast<const TMAC_GLOBAL uint32_t*>(scq + boff);
                    r0 = p32[0];
                    if (ZP) r1 = p32[1];
                }
            }
            f.t0 = r0; f.t1 = r1;
            p_st += wpq;
            if (p_st >= nst) { p_st = h; p_q += stride; }
        }
    };
    issue(f0); issue(f1);
    if (RING == 4) { issue(f2); issue(f3); }

    // ---- 2. tables of the live rows into LDS (k_gemv_quad, LUTSRC == 0) ---------------------------------------------------------
#pragma unroll 1
    for (int r = 0; r < nr; ++r) {
        const int n = n0 + r;
        uint4* tab = lds + (size_t)r * row_u4;
        float* l_ls = reinterpret_cast<float*>(tab + 4 * tstride);
        float* l_lb = l_ls + GP;
        const uint4* src = reinterpret_cast<const uint4*>(a.qlut_lds) + (size_t)n * 4 * a.tstride;
#pragma unroll
        for (int j4 = 0; j4 < 4; ++j4) {
            for (int u = tid; u < nu; u += FT) {
                uint4 v = src[j4 * a.tstride + u];
                v.x ^= 0x80808080u; v.y ^= 0x80808080u; v.z ^= 0x80808080u; v.w ^= 0x80808080u;
                tab[j4 * tstride + u] = v;
            }
            for (int u = nu + tid; u < nst * 64; u += FT) tab[j4 * tstride + u] = make_uint4(0u, 0u, 0u, 0u);
        }
        if (SM == 2) { if (tid == 0) { l_ls[0] = a.lut_scales[n]; l_lb[0] = a.lut_biases[n]; } }
        else {
            for (int i = tid; i < G; i += FT) { l_ls[i] = __fmul_rn(0.5f, a.lut_scales[(size_t)n * G + i]); l_lb[i] = __fmul_rn(0.5f, a.lut_biases[(size_t)n * G + i]); }
            for (int i = G + tid; i < GP; i += FT) { l_ls[i] = 0.f; l_lb[i] = 0.f; }
        }
    }
    __syncthreads();

    // ---- 3. stream this wave's quads ----------------------------------------------------------------------------------------------
    float cacc[R];
    int32_t iacc[R][BITS];
    auto reset_acc = [&]() {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            cacc[r] = 0.f;
#pragma unroll
            for (int pl = 0; pl < BITS; ++pl) iacc[r][pl] = 0;
        }
    };
    reset_acc();
    CSel<BITS> sel;
    c_selectors<BITS, SM>(sel, lane);
    uint32_t k3 = 0x03020100u;
    asm volatile("" : "+v"(k3));     // keep the selector constant in a VGPR (operand of v_and_or_b32)

    auto compute = [&](const RFrag<BITS>& f, int st, int Mw_m, int lq) {
        float sc0 = 0.f, zr0 = 0.f, sc1 = 0.f, zr1 = 0.f;
        if (SM == 0) {
            r_decode<ZP, SCF16>(f.c.s0, f.c.s1, sc0, zr0);
            r_decode<ZP, SCF16>(two_sg ? f.t0 : f.c.s0, two_sg ? f.t1 : f.c.s1, sc1, zr1);
        }
        const int o = 4 * lq + (lane & 3);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (r < nr) {
                const uint4* tab = lds + (size_t)r * row_u4;
                const float* l_ls = reinterpret_cast<const float*>(tab + 4 * tstride);
                int32_t* tap_row = (SM == 0 && a.tap && o < Mw_m) ? a.tap + ((size_t)(n0 + r) * Mw_m + o) * G : nullptr;
                r_compute<BITS, ZP, SM>(f.c, tab, tstride, l_ls, l_ls + GP, st * 64, lane16, lk4, sel, k3, sc0, zr0, sc1, zr1, cacc[r], iacc[r], tap_row, G);
            }
        }
    };

    // reduce one quad over the 64 lanes (finish_quad of k_gemv_quad, per live row), combine the wpq waves through LDS in wave order
    // (double-buffered by iteration parity), store 4 outputs per row
    int parity = 0;
    auto finish_quad = [&](bool have, const FusedMat& M, int lq) {
        float* red = l_red + parity * (R * NWV * 16);
        const int o = 4 * lq + lane;
        if (SM != 2) {
            float acc[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                float v = 0.f;
                if (have && r < nr) {
                    v = cacc[r];
                    v = __fadd_rn(v, dpp_f<0x124>(v));     // lanes with the same beta: rotate by 4, 8 within the row
                    v = __fadd_rn(v, dpp_f<0x128>(v));
                    v = q_xor_add_f(v);
                }
                acc[r] = v;
            }
            if (wpq == 1) {
#pragma unroll
                for (int r = 0; r < R; ++r)
                    if (have && r < nr && lane < 4 && o < M.Mw) st_out(M.C, a.out_f16, (size_t)(n0 + r) * M.Mw + o, acc[r]);
            } else {
                if (lane < 4) {
#pragma unroll
                    for (int r = 0; r < R; ++r) if (r < nr) red[(r * NWV + w) * 4 + lane] = acc[r];
                }
                __syncthreads();
                if (have && h == 0 && lane < 4 && o < M.Mw) {
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        if (r < nr) {
                            float t = red[(r * NWV + w) * 4 + lane];
                            for (int ww = 1; ww < wpq; ++ww) t = __fadd_rn(t, red[(r * NWV + w + ww) * 4 + lane]);
                            st_out(M.C, a.out_f16, (size_t)(n0 + r) * M.Mw + o, t);
                        }
                    }
                }
            }
        } else {
            int32_t* redi = reinterpret_cast<int32_t*>(red);
            int32_t tot[R][BITS];
#pragma unroll
            for (int r = 0; r < R; ++r) {
#pragma unroll
                for (int pl = 0; pl < BITS; ++pl) {       // every lane holds a partial of row lane & 3: rotate by 4, 8 within the row, then rows
                    uint32_t v = (have && r < nr) ? (uint32_t)iacc[r][pl] : 0u;
                    v += dpp_u<0x124>(v);
                    v += dpp_u<0x128>(v);
                    v = q_xor_add_u(v);
                    tot[r][pl] = (int32_t)v;
                }
            }
            if (wpq > 1) {
                if (lane < 4) {
#pragma unroll
                    for (int r = 0; r < R; ++r)
#pragma unroll
                        for (int pl = 0; pl < BITS; ++pl) if (r < nr) redi[((r * NWV + w) * 4 + lane) * 4 + pl] = tot[r][pl];
                }
                __syncthreads();
            }
            if (have && h == 0 && lane < 4 && o < M.Mw) {
                const float wsc = ld_scale(M.SC, a.sc_f16, o / (M.Mw / a.s.m_groups));
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    if (r < nr) {
                        const float* l_ls = reinterpret_cast<const float*>(lds + (size_t)r * row_u4 + 4 * tstride);
                        float acc = 0.f;
#pragma unroll
                        for (int pl = 0; pl < BITS; ++pl) {
                            int32_t cb = tot[r][pl];
                            for (int ww = 1; ww < wpq; ++ww) cb += redi[((r * NWV + w + ww) * 4 + lane) * 4 + pl];
                            if (a.tap) a.tap[((size_t)(n0 + r) * M.Mw + o) * BITS + pl] = cb;
                            const float t = __fmul_rn((float)cb, alpha_of(pl));
                            acc = (pl == 0) ? t : __fadd_rn(acc, t);
                        }
                        const float v = __fadd_rn(__fmul_rn(acc, l_ls[0]), __fmul_rn(l_ls[GP], 0.5f));
                        st_out(M.C, a.out_f16, (size_t)(n0 + r) * M.Mw + o, __fmul_rn(v, wsc));
                    }
                }
            }
        }
        parity ^= 1;
        reset_acc();
    };

    // The fragment ring is consumed in issue order by a loop unrolled over the ring (k_gemv_quad).  A quad is closed when the cursor
    // leaves it; every wave closes the same number of quads, with or without work, so the barriers inside finish_quad stay matched.
    int c_it = 0, c_st = h, lq = 0;
    bool have = slot0 < total_q && h < nst;
    if (have) { seek(cc, slot0); lq = slot0 - cc.base; }
    if ((int)blockIdx.x * IPI < total_q) {      // uniform: this workgroup has at least one quad iteration
#define RSTEP(F)                                                                                              \
        while (!(have && c_st < nst)) {                                                                       \
            finish_quad(have, cc.m, lq);                                                                      \
            ++c_it;                                                                                           \
            if ((int)blockIdx.x * IPI + c_it * stride >= total_q) goto r_done;                                \
            const int gq = slot0 + c_it * stride;                                                             \
            have = gq < total_q && h < nst;                                                                   \
            if (have) { seek(cc, gq); lq = gq - cc.base; }                                                    \
            c_st = h;                                                                                         \
        }                                                                                                     \
        compute(F, c_st, cc.m.Mw, lq);                                                                        \
        issue(F);                                                                                             \
        c_st += wpq;
        for (;;) {
            RSTEP(f0)
            RSTEP(f1)
            if (RING == 4) {
                RSTEP(f2)
                RSTEP(f3)
            }
        }
#undef RSTEP
    }
r_done:;
}

// ---------------------------------------------------------------------------------------------------------------------------------
#if !defined(TMAC_ROWS_BITS)
#error "compile with -DTMAC_ROWS_BITS=1..4 (one translation unit per weight width keeps the build parallel)"
#endif

// This unit's launcher (declared in tmac_kernels.h; launch_gemv_rows, tmac_launch.cpp, plans the launches and picks the unit).
template <int BITS>
hipError_t launch_gemv_rows_unit(const RowsArgs& a, const RowsLaunch& l, hipStream_t st) {
    // scale flavour: unified scale (one scalar read per output, the dtype a run-time flag), or per-group scales by zero points and dtype
    auto flavour = [&](auto&& f) {
        if (a.s.m_groups >= 1) return f(std::false_type{}, std::false_type{}, std::integral_constant<int, 2>{});
        return sel_bool(a.s.zero_point != 0, [&](auto ZP) { return sel_bool(a.sc_f16 != 0, [&](auto SCF16) {
            return f(ZP, SCF16, std::integral_constant<int, 0>{});
        }); });
    };
    return flavour([&](auto ZP, auto SCF16, auto SM) { return sel_int<2, 4, 8>(l.R, [&](auto R) {
        static_assert(rows_inst_exists(R), "k_gemv_rows: row capacity 2, 4 or 8");
        static size_t allowed = 0;      // per kernel: the largest footprint of a capacity is allowed once
        return launch_lds_once(allowed, ROWS_LDS_MAX, k_gemv_rows<BITS, ZP, SCF16, SM, R>, dim3(l.gx, l.gy), dim3(ROWS_FT), l.lds_bytes, st, a);
    }); });
}
template hipError_t launch_gemv_rows_unit<TMAC_ROWS_BITS>(const RowsArgs&, const RowsLaunch&, hipStream_t);

}  // namespace tmac
