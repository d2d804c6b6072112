// tmac_experts_router.hip -- k_experts_router: the router of a mixture-of-experts layer in one launch.  For every token row n of x [N][K] and
// a dense router matrix Wr [E][K]: logit[n][e] = sum_k x[n][k] Wr[e][k] (fp32), p = softmax(logit[n][:]), the S experts of largest logit
// into ids[n][0..S) -- largest first, the lower id among equals -- and gates[n][s] = p[ids[n][s]], optionally over the sum of the S
// selected.  ids int32 [N][S] and gates fp32 [N][S] are what k_gemv_experts, k_experts_route and k_experts_combine read.  DESIGN.md 4.19.
//
//   split     one workgroup of 16 waves per tile of 32 tokens.  Wave w = slice * ctiles + column tile: a column tile is 32 experts, a slice
//             a run of 64-value K steps (experts_router_plan: by (K, E) alone, so a token's bits are those of its N = 1 call).
//   logits    on the matrix cores, 32 tokens x 32 experts per wave: v_mfma_f32_32x32x16_f16 when x and Wr are both fp16 (HH), else
//             v_mfma_f32_32x32x2_f32 with an fp16 operand widened in registers.  Lane (kb, r) holds token row r as A and expert row r as B
//             and feeds both from global memory with 16-byte loads: of a CHUNK of K -- one 128-byte line of an fp16 (HH) or fp32 row -- the
//             lane owns the half kb, contiguous, and MFMA m of the chunk takes the m-th 8 (HH) / the m-th single value of every lane.  A
//             and B share the mapping, so the k order inside an instruction never shows.  The next chunk's loads are issued before this
//             chunk's MFMAs.  Rows beyond N and experts beyond E are zero registers: nothing is loaded for them, nothing stored.
//   reduce    every wave writes its 32 x 32 partial to LDS [slice][32][e_pad]; after one barrier a logit is the sum over the slices in
//             slice order.  No atomics.
//   select    wave w takes the token rows w, w + 16; lane l holds the logits e = l + 64 j, j < 4.  The order is that of an integer key --
//             the fp32 bits made monotone, -0 as +0 -- so a NaN has a place in it (above +Inf with the sign clear, below -Inf with it
//             set).  A round: the wave's largest live key by DPP, then the lowest expert that holds it by ballots, j-major; that expert
//             leaves the order.  S rounds give S distinct ids in [0, E) whatever the bits.  The row maximum is round 0's key, the row sum
//             one DPP reduction of the expf values, the divisions are true divisions.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>

#include "tmac_kernels.h"
#include "tmac_select.h"

namespace tmac {

typedef _Float16 rt_h8_t __attribute__((ext_vector_type(8)));
typedef float rt_16f_t __attribute__((ext_vector_type(16)));

struct RouterGeom { int ctiles, slices, steps, e_pad; };      // of experts_router_plan

// what a lane holds of one chunk of a row, as loaded
struct RouterFrag { uint4 q[4]; };

// the lane's part of a chunk at value k of `row`: HH 32 halves; else 16 values, 32 or 64 bytes.  !live: zeros, nothing is read.
template <bool HH>
__device__ __forceinline__ void router_load(RouterFrag& f, const char* row, bool live, bool f16, int k) {
    const uint4* p = reinterpret_cast<const uint4*>(row + (size_t)k * (f16 ? 2 : 4));
    const uint4 z = make_uint4(0, 0, 0, 0);
    const bool four = HH || !f16;
    f.q[0] = z; f.q[1] = z; f.q[2] = z; f.q[3] = z;
    if (live) {
        f.q[0] = p[0]; f.q[1] = p[1];
        if (four) { f.q[2] = p[2]; f.q[3] = p[3]; }
    }
}

__device__ __forceinline__ uint32_t router_word(const RouterFrag& f, int i) {      // (i: a constant after unrolling)
    const uint4 q = f.q[i >> 2];
    return (i & 3) == 0 ? q.x : (i & 3) == 1 ? q.y : (i & 3) == 2 ? q.z : q.w;
}

// value i (of 16) of a fragment of the fp32 arithmetic: as stored, or an fp16 widened (exact)
__device__ __forceinline__ float router_value(const RouterFrag& f, bool f16, int i) {
    if (!f16) return __uint_as_float(router_word(f, i));
    const uint32_t wd = router_word(f, i >> 1);
    return __half2float(__ushort_as_half((unsigned short)((i & 1) ? wd >> 16 : wd & 0xffffu)));
}

template <bool HH>
__device__ __forceinline__ void router_mma(rt_16f_t& acc, const RouterFrag& x, const RouterFrag& wr, bool x_f16, bool w_f16) {
    if constexpr (HH) {
#pragma unroll
        for (int m = 0; m < 4; ++m)
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(rt_h8_t, x.q[m]), __builtin_bit_cast(rt_h8_t, wr.q[m]), acc, 0, 0, 0);
    } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(router_value(x, x_f16, i), router_value(wr, w_f16, i), acc, 0, 0, 0);
    }
}

// all-lanes reduction of a wave, the same bits in every lane: xor 1, xor 2, half-row mirror, row mirror inside the rows of 16 (DPP), then
// the four rows through scalar registers
template <class Op>
__device__ __forceinline__ uint32_t router_wave_all(uint32_t v, Op op) {
    v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false));      // quad_perm [1, 0, 3, 2]
    v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false));      // quad_perm [2, 3, 0, 1]
    v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, false));     // row_half_mirror
    v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, false));     // row_mirror
    const uint32_t r0 = __builtin_amdgcn_readlane((int)v, 0), r1 = __builtin_amdgcn_readlane((int)v, 16);
    const uint32_t r2 = __builtin_amdgcn_readlane((int)v, 32), r3 = __builtin_amdgcn_readlane((int)v, 48);
    return op(op(r0, r1), op(r2, r3));
}
__device__ __forceinline__ uint32_t router_max_u32(uint32_t a, uint32_t b) { return a > b ? a : b; }
__device__ __forceinline__ uint32_t router_add_f32(uint32_t a, uint32_t b) { return __float_as_uint(__fadd_rn(__uint_as_float(a), __uint_as_float(b))); }

// fp32 bits -> a key whose unsigned order is the values' (-0 = +0; NaN: beyond the infinity of its sign), and back
__device__ __forceinline__ uint32_t router_key(float v) {
    uint32_t u = __float_as_uint(v);
    if (u == 0x80000000u) u = 0;
    return (u >> 31) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float router_unkey(uint32_t k) { return __uint_as_float((k >> 31) ? (k ^ 0x80000000u) : ~k); }

template <bool HH>
__global__ __launch_bounds__(ROUTER_FT) void k_experts_router(const ExpertsRouterArgs a, const RouterGeom g) {
    extern __shared__ float part[];                       // [slices][32][e_pad]
    const int tid = threadIdx.x, w = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int n0 = blockIdx.x * ROUTER_TOKENS;

    // ---- logits: this wave's 32 x 32 tile over its K slice ------------------------------------------------------------------------------
    if (w < g.ctiles * g.slices) {
        const int ct = w % g.ctiles, sl = w / g.ctiles, kb = lane >> 5, r = lane & 31;
        const int n = n0 + r, e = ct * 32 + r;
        const bool x_live = n < a.N, w_live = e < a.E;
        const char* xrow = reinterpret_cast<const char*>(a.x) + (x_live ? (size_t)n * a.K * (a.x_f16 ? 2 : 4) : 0);
        const char* wrow = reinterpret_cast<const char*>(a.Wr) + (w_live ? (size_t)e * a.K * (a.w_f16 ? 2 : 4) : 0);
        constexpr int CK = HH ? 64 : 32, CPS = ROUTER_KSTEP / CK;          // values of a chunk; chunks per K step
        const int c_lo = sl * g.steps * CPS, c_end = c_lo + g.steps * CPS, c_hi = c_end < a.K / CK ? c_end : a.K / CK;
        rt_16f_t acc;
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[v] = 0.f;
        RouterFrag xa, wa, xb, wb;
        auto load = [&](RouterFrag& fx, RouterFrag& fw, int c) {
            const int k = c * CK + kb * (CK / 2);
            router_load<HH>(fx, xrow, x_live, a.x_f16, k);
            router_load<HH>(fw, wrow, w_live, a.w_f16, k);
        };
        if (c_lo < c_hi) load(xa, wa, c_lo);
        for (int c = c_lo; c < c_hi; c += 2) {              // (uniform: two chunks a trip, the other buffer loading under the MFMAs)
            const bool two = c + 1 < c_hi;
            if (two) load(xb, wb, c + 1);
            router_mma<HH>(acc, xa, wa, a.x_f16, a.w_f16);
            if (two) {
                if (c + 2 < c_hi) load(xa, wa, c + 2);
                router_mma<HH>(acc, xb, wb, a.x_f16, a.w_f16);
            }
        }
        // D[i][j]: register v of lane (kb, j) is row i = 8 (v / 4) + 4 kb + v % 4
        float* pt = part + (size_t)sl * ROUTER_TOKENS * g.e_pad + e;
#pragma unroll
        for (int v = 0; v < 16; ++v) pt[(8 * (v >> 2) + 4 * kb + (v & 3)) * g.e_pad] = acc[v];
    }
    __syncthreads();

    // ---- softmax and top-S: a wave per token row ------------------------------------------------------------------------------------------
    for (int t = w; t < ROUTER_TOKENS && n0 + t < a.N; t += ROUTER_NWV) {
        const int n = n0 + t;
        float l[4];
        uint32_t key[4];
        bool alive[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = lane + 64 * j;
            alive[j] = e < a.E;
            float v = 0.f;
            if (alive[j]) {
                const float* p = part + t * g.e_pad + e;
                v = p[0];
                for (int s = 1; s < g.slices; ++s) v = __fadd_rn(v, p[(size_t)s * ROUTER_TOKENS * g.e_pad]);      // slice order
                if (a.logits) a.logits[(size_t)n * a.E + e] = v;
            }
            l[j] = v;
            key[j] = router_key(v);
        }
        auto live_max = [&]() {
            uint32_t m = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) m = alive[j] ? router_max_u32(m, key[j]) : m;
            return router_wave_all(m, router_max_u32);
        };
        const float mx = router_unkey(live_max());
        float p[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) p[j] = alive[j] ? expf(__fsub_rn(l[j], mx)) : 0.f;
        const float lane_sum = __fadd_rn(__fadd_rn(__fadd_rn(p[0], p[1]), p[2]), p[3]);
        const float sum = __uint_as_float(router_wave_all(__float_as_uint(lane_sum), router_add_f32));

        int my_id = 0;
        float my_gate = 0.f, total = 0.f;
        for (int s = 0; s < a.S; ++s) {                      // S <= E: a live expert is left in every round
            const uint32_t m = live_max();
            int wj = 0, wl = 0;
#pragma unroll
            for (int j = 3; j >= 0; --j) {                   // the lowest expert that holds m: j-major, then the lowest lane
                const unsigned long long has = __ballot(alive[j] && key[j] == m);
                if (has) { wj = j; wl = (int)__builtin_ctzll(has); }
            }
            wj = __builtin_amdgcn_readfirstlane(wj); wl = __builtin_amdgcn_readfirstlane(wl);
            const float pj = wj == 0 ? p[0] : wj == 1 ? p[1] : wj == 2 ? p[2] : p[3];
            const float gate = __fdiv_rn(__uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(pj), wl)), sum);
            total = __fadd_rn(total, gate);
            if (lane == s) { my_id = wl + 64 * wj; my_gate = gate; }
#pragma unroll
            for (int j = 0; j < 4; ++j) alive[j] = alive[j] && !(lane == wl && j == wj);
        }
        if (lane < a.S) {
            a.ids[(size_t)n * a.S + lane] = my_id;
            a.gates[(size_t)n * a.S + lane] = a.renorm ? __fdiv_rn(my_gate, total) : my_gate;
        }
    }
}

hipError_t launch_experts_router(const ExpertsRouterArgs& a, const ExpertsRouterPlan& p, hipStream_t st) {
    if (p.why || !a.Wr || !a.x || !a.ids || !a.gates) return hipErrorInvalidValue;
    if (p.waves < 1 || p.waves > ROUTER_NWV || p.waves != p.ctiles * p.slices || p.e_pad != 32 * p.ctiles || p.e_pad < a.E ||
        (long long)p.slices * p.steps * ROUTER_KSTEP < a.K || (long long)(p.slices - 1) * p.steps * ROUTER_KSTEP >= a.K ||
        (long long)p.gx * ROUTER_TOKENS < a.N || p.lds_bytes != sizeof(float) * p.slices * ROUTER_TOKENS * p.e_pad)
        return hipErrorInvalidValue;                      // (a plan of another call shape)
    const RouterGeom g{p.ctiles, p.slices, p.steps, p.e_pad};
    return sel_bool(a.x_f16 && a.w_f16, [&](auto HH) {
        return launch_lds(k_experts_router<decltype(HH)::value>, dim3(p.gx), dim3(ROUTER_FT), p.lds_bytes, st, a, g);
    });
}

}  // namespace tmac
