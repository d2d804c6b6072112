// tmac_experts.hip -- k_gemv_experts: the top-k expert GEMVs of a mixture-of-experts layer, the expert of every slot read on the device.
//
// Work decomposition of k_gemv_quad / k_gemv_rows: a WAVE owns a row quad, its 64 lanes hold the 64 units of a 64-unit step; persistent
// eight-wave workgroups walk their item list, 1 / 2 / 4 waves per quad splitting the steps (combined through LDS in wave order).  The
// item is built from tmac_chain_core.h: CFrag / c_issue for the weight fragment (scales in the fragment), c_selectors, and c_compute's
// lookups + MFMA adder + per-act-group fp32 chain in its two-scale-group form (the second scale word is fetched beside the fragment
// only where gs = 64, decided at run time as k_gemv_rows does; for gs >= 128 it repeats the first and the bits are the plain item's).
// What is new: WHICH matrix an item streams is not in the argument block.  A bank is a device table of E interchangeable matrices
// (ExpertEntry: QUAD-layout weights + scales); the launch gets ids[S] on the device and up to two banks that share them (gate / up).
//   item      SLOTS: (slot, bank, row quad) -- C[bank][slot][:] = W_bank[ids[slot]] . x_row(slot)
//             COMBINE: a row quad of the one bank; its wave walks the S slots in turn and keeps acc = acc + g[s] * y_s (two roundings
//             per slot, slot order, from 0) in a register: one store per output, no atomics, no second kernel.  y_s is finished exactly
//             as SLOTS finishes it (lane reduction, then the quad's waves through LDS in wave order), so COMBINE is reproducible bit
//             for bit from the SLOTS outputs.
//   selection a wave reads ids[slot] and then the bank's entry with wave-uniform loads and forms the fragment's buffer resource and scale
//             pointer from them.  One unsigned compare decides whether the slot is EMPTY (id outside [0, E); -1 is the documented
//             value): no address is formed from such an id, its SLOTS row is stored as zeros, it adds nothing to a COMBINE output.
//   x_row(s)  row 0 for every slot (lut_rows = 1: gate / up read the token's one vector, ONE set of tables in LDS) or row s (lut_rows = S).
// LUTSRC 0: the tables are COPIED from the workspace's half-table image exactly as k_gemv_rows / k_gemv_quad (LUTSRC == 0) copy them (xor
// 0x80808080 for the MFMA adder, scales halved, zero tables between nu and the end of the last step).  The first weight fragments
// are issued before the copy, and the copy takes the rows four at a time -- 16 table loads per thread in flight before the first LDS
// store -- so a call's rows cost one or two memory latencies, not one each (the cost k_gemv_rows measured).
// LUTSRC 1: the tables are BUILT in the launch from the call's activation rows, by the constructor of tmac_lut_build.h; LUTSRC 2: from
// x = gate(in) * in2 (xf_gate_mul, the gate a run-time value: silu, relu^2, tanh-GELU), the GLU between gate / up and down.  The
// lut_rows * K / 8 pairs (8 activations, two tables) are ONE flat index over the 512 threads -- the rows are contiguous, a lane holds a
// pair, the 8 adjacent lanes of an act group of 64 never straddle a row (K is a multiple of 64) -- walked in batches of EXPERTS_LUT_NB
// (4; 2 behind a GLU) pairs per thread; lanes past the end are clamped to the last pair and their stores dropped.  Order of the memory stream (k_gemv_quad's):
// the first batch's activation loads, a wait for those registers alone, the weight ring, then the build on the VALU while the fragments
// fly, the LDS stores and an LDS-only barrier.  Later batches' loads queue behind the ring.  The LDS image is the copy's to the bit, so
// everything behind the barrier is the same code, and a slot's bits do not depend on which form made its tables.
// No waits between workgroups, no spins, no atomics.  DESIGN.md 4.17.
#define TMAC_LUT_SINGLE_F32 1      // (this unit is built without packed-fp32 instructions: tmac_lut_build.h)
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>

#include "tmac_core.h"
#include "tmac_kernels.h"
#include "tmac_chain_core.h"
#include "tmac_quad_core.h"
#include "tmac_lut_build.h"
#include "tmac_select.h"

namespace tmac {

template <int BITS>
struct EFrag {
    CFrag<BITS> c;
    uint32_t t0, t1;      // gs = 64 only: scale (, zero) of the lane's SECOND act group of the step (layout of c.s0, c.s1)
};

// where a (work item, slot) lies: which output, and -- live alone -- which matrix it streams
struct ECur {
    bool in_range;        // the item exists (the tail of the last pass does not)
    bool valid;           // ... and its slot names an expert of its bank
    bool live;            // ... and this wave has steps of it
    int slot, bank, lq;   // lq: row quad inside the bank's matrices
    __amdgpu_buffer_rsrc_t rs;         // the expert's weights
    const TMAC_GLOBAL char* scq;       // first scale group of the quad
    int woff;                          // byte offset of the quad's first fragment
};

// Pairs per thread and batch of the in-launch build, from the register figures (profiles/r30_experts_fused_resources.txt).  LUTSRC 1: 4 --
// 32 fp32 registers of activations beside the weight ring, 82 - 107 VGPRs where the copy form (16 table loads in flight) has 109 - 133; one
// batch covers 16384 activations.  LUTSRC 2 holds both operands of the GLU until the ring is out: with 4 pairs every instantiation passed
// 128 VGPRs (135 - 160) and lost the second workgroup per CU; with 2 they have 83 - 108.  No instantiation uses scratch.
template <int LUTSRC> constexpr int EXPERTS_LUT_NB = LUTSRC == 2 ? 2 : 4;

template <int BITS, bool ZP, bool SCF16, int MODE, int LUTSRC = 0>
__global__ __launch_bounds__(EXPERTS_FT) void k_gemv_experts(ExpertsArgs a) {
    extern __shared__ uint4 lds[];
    constexpr int NWV = EXPERTS_NWV, FT = EXPERTS_FT;
    const int tid = threadIdx.x, w = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int nu = a.nu, nst = a.nst, G = a.G, S = a.S, LR = a.lut_rows;
    const int tstride = nst * 64 + 1;                                 // whole steps: units past K hold zero tables
    const int GP = nst * 32;                                          // act groups of the padded steps (>= G)
    const int row_u4 = 4 * tstride + GP / 2;                          // per row: [4][tstride] uint4 tables | ls / 2 [GP] | lb / 2 [GP]
    float* l_red = reinterpret_cast<float*>(lds + (size_t)LR * row_u4);   // [2][NWV][4 rows]: partials of the waves of a quad
    const int wpq = a.wpq, IPI = NWV / wpq;
    const bool two_sg = a.gs_shift < 2;                               // gs = 64: the lane's two act groups have a scale group each
    const int Q0 = a.b[0].q_end, QT = a.b[a.nbanks - 1].q_end;        // row quads of bank 0 / of all banks
    const int total = MODE == EXPERTS_COMBINE ? QT : S * QT;
    const int nsub = MODE == EXPERTS_COMBINE ? S : 1;                 // slots a wave walks per item
    constexpr int per = ZP ? 2 : 1, esz = SCF16 ? 2 : 4;

    uint32_t lane16 = (uint32_t)lane * 16u;                           // the lane's 16 bytes of a table row / weight block
    asm volatile("" : "+v"(lane16));
    uint32_t lk4 = 4u * (uint32_t)(2 * (lane & 12) + 2 * (lane >> 4));   // the lane's two act groups inside a step's 32
    asm volatile("" : "+v"(lk4));

    const int slot0 = (int)blockIdx.x * IPI + w / wpq, h = w % wpq, stride = (int)gridDim.x * IPI;

    // ---- 0. LUTSRC >= 1: the activations of the first batch of pairs leave first (LUTSRC 2: both operands of the GLU) ------------------
    constexpr int NB = EXPERTS_LUT_NB<LUTSRC>;
    const int PR = 4 * nu, NPAIR = LR * PR;                           // pairs of a row, of the call
    [[maybe_unused]] float xr[LUTSRC != 0 ? NB * 8 : 1], xa[LUTSRC == 2 ? NB * 8 : 1];
    auto lut_load = [&](int b) {
        if constexpr (LUTSRC != 0) {
            auto ld = [&](const void* src, float* x) {                 // [lut_rows][K] contiguous: pair f of the call is pair f of the buffer
                if (a.act_f16) {
                    uint4 v[NB];
#pragma unroll
                    for (int r = 0; r < NB; ++r) v[r] = reinterpret_cast<const uint4*>(src)[min((b * NB + r) * FT + tid, NPAIR - 1)];
#pragma unroll
                    for (int r = 0; r < NB; ++r) {
                        const uint32_t wd[4] = {v[r].x, v[r].y, v[r].z, v[r].w};
                        const lut_f32x8 t = lut_unpack_f16v(wd);
#pragma unroll
                        for (int i = 0; i < 8; ++i) x[r * 8 + i] = t[i];
                    }
                } else {
#pragma unroll
                    for (int r = 0; r < NB; ++r) {
                        const lut_f32x8 t = lut_ld8v(src, false, 0, min((b * NB + r) * FT + tid, NPAIR - 1));
#pragma unroll
                        for (int i = 0; i < 8; ++i) x[r * 8 + i] = t[i];
                    }
                }
            };
            ld(a.B, xr);
            if constexpr (LUTSRC == 2) ld(a.in2, xa);
        }
    };
    lut_load(0);

    // ---- device-side selection: (item gq, slot `sub` of a COMBINE item) -> output position and, for a live one, the expert's pointers.
    //      Everything here is wave-uniform: scalar loads of ids[slot] and of the bank's 16-byte entry, nothing else touches the id.
    auto resolve = [&](int gq, int sub, ECur& c) {
        c.in_range = gq < total; c.valid = false; c.live = false;
        c.slot = 0; c.bank = 0; c.lq = 0;
        if (!c.in_range) return;
        int slot = sub, q = gq;
        if (MODE == EXPERTS_SLOTS) { slot = gq / QT; q = gq - slot * QT; }
        const int bank = q >= Q0 ? 1 : 0;
        c.slot = slot; c.bank = bank; c.lq = q - (bank ? Q0 : 0);
        const uint32_t id = (uint32_t)uni(a.ids[slot]);
        if (id >= (uint32_t)(bank ? a.b[1].E : a.b[0].E)) return;    // empty slot: no address is formed from its id
        c.valid = true;
        if (h >= nst) return;
        const ExpertEntry* tab = bank ? a.b[1].tab : a.b[0].tab;
        const uint4* W = uni(tab[id].W);
        const char* SC = uni(reinterpret_cast<const char*>(tab[id].SC));
        c.rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint4*>(W), (short)0, 0x7fffffff, 0x00020000);
        c.scq = (const TMAC_GLOBAL char*)SC + (size_t)c.lq * (size_t)(a.nsg * 4 * per * esz);
        c.woff = c.lq * nst * (BITS * 1024);
        c.live = true;
    };

    // ---- 1. this wave's work: items slot0, slot0 + stride, ...; of each its slots in turn; of each slot steps h, h + wpq, ...  The
    //         first fragments are issued BEFORE the table copy, so the weight stream overlaps it -------------------------------------
    constexpr int RING = (BITS <= 2) ? 4 : 2;                         // weight fragments in flight per wave
    EFrag<BITS> f0, f1, f2, f3;
    int p_it = 0, p_sub = 0, p_st = h;                                // prefetch cursor
    bool p_done = h >= nst;
    ECur pc;
    auto p_seek = [&]() {                                             // to the next live (item, slot) at or behind the cursor
        while (!p_done) {
            const int gq = slot0 + p_it * stride;
            if (gq >= total) { p_done = true; break; }
            resolve(gq, p_sub, pc);
            if (pc.live) break;
            if (++p_sub >= nsub) { p_sub = 0; ++p_it; }
        }
    };
    auto issue = [&](EFrag<BITS>& f) {
        if (!p_done) {
            c_issue<BITS, ZP, SCF16, 0>(f.c, pc.rs, pc.woff, pc.scq, a.nsg, a.gs_shift, nu, p_st, lane, lane16);
            uint32_t r0 = 0, r1 = 0;
            if (two_sg) {           // clamped, not predicated: groups past K meet zero tables and zero LUT scales
                const int c0 = 4 * (lane & 12) + 4 * (lane >> 4) + 2;
                const uint32_t sg = min((uint32_t)p_st * (64u >> a.gs_shift) + (uint32_t)(c0 >> a.gs_shift), (uint32_t)a.nsg - 1u);
                c_ld_scale2<ZP, SCF16>(pc.scq + (sg * 4 + (lane & 3)) * (per * esz), r0, r1);
            }
            f.t0 = r0; f.t1 = r1;
            p_st += wpq;
            if (p_st >= nst) {
                p_st = h;
                if (++p_sub >= nsub) { p_sub = 0; ++p_it; }
                p_seek();
            }
        }
    };
    p_seek();
    if constexpr (LUTSRC != 0) {      // wait for the activation registers alone (the empty asm reads them), THEN the ring: k_gemv_quad's `early`
#pragma unroll
        for (int i = 0; i < NB * 8; ++i) {
            asm volatile("" :: "v"(xr[i]));
            if constexpr (LUTSRC == 2) asm volatile("" :: "v"(xa[i]));
        }
    }
    issue(f0); issue(f1);
    if (RING == 4) { issue(f2); issue(f3); }

    // ---- 2. tables of the call's rows into LDS (k_gemv_quad, LUTSRC == 0), four rows' loads in flight before the first store ----------
    if constexpr (LUTSRC == 0) {
        const uint4* img = reinterpret_cast<const uint4*>(a.qlut_lds);
        auto row_tab = [&](int r) { return lds + (size_t)r * row_u4; };
#pragma unroll 1
        for (int r0 = 0; r0 < LR; r0 += 4) {
#pragma unroll 1
            for (int i = tid; i < GP; i += FT) {
                float ls[4], lb[4];
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    const bool on = r0 + rr < LR && i < G;
                    ls[rr] = on ? a.lut_scales[(size_t)(r0 + rr) * G + i] : 0.f;
                    lb[rr] = on ? a.lut_biases[(size_t)(r0 + rr) * G + i] : 0.f;
                }
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    if (r0 + rr < LR) {
                        float* l_ls = reinterpret_cast<float*>(row_tab(r0 + rr) + 4 * tstride);
                        l_ls[i] = __fmul_rn(0.5f, ls[rr]); l_ls[GP + i] = __fmul_rn(0.5f, lb[rr]);
                    }
                }
            }
#pragma unroll 1
            for (int u = tid; u < nst * 64; u += FT) {
                uint4 v[4][4];
                const int uc = min(u, nu - 1);                         // clamped, not predicated: the loads of a batch leave back to back
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
#pragma unroll
                    for (int j4 = 0; j4 < 4; ++j4) {
                        v[rr][j4] = make_uint4(0u, 0u, 0u, 0u);
                        if (r0 + rr < LR) v[rr][j4] = img[((size_t)(r0 + rr) * 4 + j4) * a.tstride + uc];
                    }
                }
                const bool pad = u >= nu;                              // units past K: zero tables
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    if (r0 + rr < LR) {
                        uint4* tab = row_tab(r0 + rr);
#pragma unroll
                        for (int j4 = 0; j4 < 4; ++j4) {
                            uint4 t = v[rr][j4];
                            t.x ^= 0x80808080u; t.y ^= 0x80808080u; t.z ^= 0x80808080u; t.w ^= 0x80808080u;
                            tab[j4 * tstride + u] = pad ? make_uint4(0u, 0u, 0u, 0u) : t;
                        }
                    }
                }
            }
        }
        __syncthreads();
    } else {
        // ---- 2'. ... or built here, on the VALU while the fragments fly: batch by batch the pieces of tmac_lut_build.h on the lane's pair,
        //      into the image section 3 reads -- tables 2p, 2p + 1 = the uint4 (j4 = p & 3) of unit p >> 2; ls / 2, lb / 2 per act group
        auto lut_build = [&](int b) {
            if constexpr (LUTSRC == 2) xf_gate_mul(a.xf_kind >> 8, xr, xa);      // x = gate(in) * in2, in the registers `in` arrived in
#pragma unroll
            for (int r = 0; r < NB; ++r) {
                const int f = (b * NB + r) * FT + tid, fc = min(f, NPAIR - 1);
                int row = 0;
#pragma unroll
                for (int j = 1; j < EXPERTS_MAX_SLOTS; ++j) row += fc >= j * PR ? 1 : 0;      // (fc < LR * PR: nothing counts behind LR - 1)
                const int p = fc - row * PR;
                const float* x = xr + r * 8;
                float scales, t_scales, La, Lb;
                lut_group_scale(LUT_X8(x), scales, t_scales);
                const uint4 t = lut_tables2<true>(LUT_X8(x), t_scales, La, Lb);
                const float v = lut_chunk_sum(La, Lb);
                const float c1 = lut_group_partner(v);                  // (every lane of the act group takes part)
                if (f < NPAIR) {                                        // NPAIR % 8 == 0: an act group stores or drops as a whole
                    uint4* tab = lds + (size_t)row * row_u4;
                    tab[(p & 3) * tstride + (p >> 2)] = t;
                    if ((p & 7) == 0) {
                        float* l_ls = reinterpret_cast<float*>(tab + 4 * tstride);
                        l_ls[p >> 3] = __fmul_rn(0.5f, scales);
                        l_ls[GP + (p >> 3)] = __fmul_rn(0.5f, lut_group_bias(v, c1));
                    }
                }
            }
        };
        lut_build(0);
#pragma unroll 1
        for (int b = 1; b * (NB * FT) < NPAIR; ++b) {                   // the loads of these batches queue behind the ring
            lut_load(b);
            lut_build(b);
        }
#pragma unroll 1
        for (int r = 0; r < LR; ++r) {                                  // zero tables for units >= nu, zero scales for groups >= G
            uint4* tab = lds + (size_t)r * row_u4;
            float* l_ls = reinterpret_cast<float*>(tab + 4 * tstride);
            for (int u = nu + tid; u < nst * 64; u += FT)
#pragma unroll
                for (int j4 = 0; j4 < 4; ++j4) tab[j4 * tstride + u] = make_uint4(0u, 0u, 0u, 0u);
            for (int i = G + tid; i < GP; i += FT) { l_ls[i] = 0.f; l_ls[GP + i] = 0.f; }
        }
        c_lds_barrier();              // LDS only: __syncthreads() carries vmcnt(0) and would drain the ring
    }

    // ---- 3. stream this wave's items ----------------------------------------------------------------------------------------------
    float cacc = 0.f;                 // the slot's partial of the lane's row
    float gacc = 0.f;                 // COMBINE: sum_s g[s] y_s of the quad's rows (lanes 0..3 of the quad's first wave)
    int32_t iacc[BITS] = {};          // (c_compute's unified-scale accumulators: unused with per-group scales)
    CSel<BITS> sel;
    c_selectors<BITS, 0>(sel, lane);
    uint32_t k3 = 0x03020100u;
    asm volatile("" : "+v"(k3));     // keep the selector constant in a VGPR (operand of v_and_or_b32)

    auto compute = [&](const EFrag<BITS>& f, int st, const ECur& c) {
        CFrag<BITS, true> g;          // the fragment with its second scale word: the first again where gs >= 128
#pragma unroll
        for (int j = 0; j < BITS; ++j) g.wq[j] = f.c.wq[j];
        g.s0 = f.c.s0; g.s1 = f.c.s1;
        g.t0 = two_sg ? f.t0 : f.c.s0; g.t1 = two_sg ? f.t1 : f.c.s1;
        const uint4* tab = lds + (size_t)(LR == 1 ? 0 : c.slot) * row_u4;
        const float* l_ls = reinterpret_cast<const float*>(tab + 4 * tstride);
        c_compute<BITS, ZP, SCF16, 0, false, false, true>(g, tab, tstride, l_ls, l_ls + GP, st * 64, lane16, lk4, sel, k3, cacc, iacc);
    };

    // close one slot of an item: reduce the quad over the 64 lanes (finish_quad of k_gemv_quad), combine the wpq waves through LDS in
    // wave order (double-buffered by parity), then store the slot's 4 outputs (SLOTS) or fold them into gacc (COMBINE; the store
    // follows the item's last slot).  An empty slot arrives with zeros everywhere: SLOTS stores them, COMBINE skips its term.
    int parity = 0;
    auto finish = [&](const ECur& c, bool last_sub) {
        float v = 0.f;
        if (c.live) {
            v = cacc;
            v = __fadd_rn(v, dpp_f<0x124>(v));     // lanes with the same beta: rotate by 4, 8 within the row
            v = __fadd_rn(v, dpp_f<0x128>(v));
            v = q_xor_add_f(v);
        }
        cacc = 0.f;
        if (wpq > 1) {
            float* red = l_red + parity * (NWV * 4);
            if (lane < 4) red[w * 4 + lane] = v;
            c_lds_barrier();
            if (h == 0 && lane < 4)
                for (int ww = 1; ww < wpq; ++ww) v = __fadd_rn(v, red[(w + ww) * 4 + lane]);
            parity ^= 1;
        }
        const int Mw = c.bank ? a.b[1].Mw : a.b[0].Mw;
        void* C = c.bank ? a.b[1].C : a.b[0].C;
        const int o = 4 * c.lq + lane;
        const bool mine = c.in_range && h == 0 && lane < 4 && o < Mw;
        if (MODE == EXPERTS_SLOTS) {
            if (mine) st_out(C, a.out_f16, (size_t)c.slot * Mw + o, v);
        } else {
            if (c.valid) gacc = __fadd_rn(gacc, __fmul_rn(a.gates[c.slot], v));
            if (last_sub) {
                if (mine) st_out(C, a.out_f16, (size_t)o, gacc);
                gacc = 0.f;
            }
        }
    };

    // The fragment ring is consumed in issue order by a loop unrolled over the ring (k_gemv_quad).  A slot is closed when the cursor
    // leaves it; every wave closes the same number of slots, with or without work, so the barriers inside finish stay matched.
    int c_it = 0, c_sub = 0, c_st = h;
    ECur cc;
    resolve(slot0, 0, cc);
    if ((int)blockIdx.x * IPI < total) {        // uniform: this workgroup has at least one item
#define ESTEP(F)                                                                                              \
        while (!(cc.live && c_st < nst)) {                                                                    \
            finish(cc, c_sub + 1 >= nsub);                                                                    \
            if (++c_sub >= nsub) {                                                                            \
                c_sub = 0; ++c_it;                                                                            \
                if ((int)blockIdx.x * IPI + c_it * stride >= total) goto e_done;                              \
            }                                                                                                 \
            resolve(slot0 + c_it * stride, c_sub, cc);                                                        \
            c_st = h;                                                                                         \
        }                                                                                                     \
        compute(F, c_st, cc);                                                                                 \
        issue(F);                                                                                             \
        c_st += wpq;
        for (;;) {
            ESTEP(f0)
            ESTEP(f1)
            if (RING == 4) {
                ESTEP(f2)
                ESTEP(f3)
            }
        }
#undef ESTEP
    }
e_done:;
}

// ---------------------------------------------------------------------------------------------------------------------------------
#if !defined(TMAC_EXPERTS_BITS)
#error "compile with -DTMAC_EXPERTS_BITS=1..4 (one translation unit per weight width keeps the build parallel)"
#endif

// This unit's launcher (declared in tmac_kernels.h; launch_gemv_experts, tmac_experts.cpp, plans the launch and picks the unit).
template <int BITS>
hipError_t launch_gemv_experts_unit(const ExpertsArgs& a, const ExpertsPlan& p, int mode, hipStream_t st) {
    return sel_bool(a.s.zero_point != 0, [&](auto ZP) { return sel_bool(a.sc_f16 != 0, [&](auto SCF16) {
        return sel_int<EXPERTS_SLOTS, EXPERTS_COMBINE>(mode, [&](auto MODE) {
            return sel_int<0, 1, 2>(a.lutsrc, [&](auto LUTSRC) {
                static_assert(experts_inst_exists(BITS, 0, MODE, LUTSRC), "k_gemv_experts: per-group scales, SLOTS or COMBINE, tables copied or built");
                static size_t allowed = 0;      // per kernel: the largest footprint is allowed once
                return launch_lds_once(allowed, ROWS_LDS_MAX, k_gemv_experts<BITS, ZP, SCF16, MODE, LUTSRC>, dim3(p.gx), dim3(EXPERTS_FT), p.lds_bytes, st, a);
            });
        });
    }); });
}
template hipError_t launch_gemv_experts_unit<TMAC_EXPERTS_BITS>(const ExpertsArgs&, const ExpertsPlan&, int, hipStream_t);

}  // namespace tmac
