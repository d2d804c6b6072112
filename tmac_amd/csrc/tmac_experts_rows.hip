// tmac_experts_rows.hip -- the two small kernels around a grouped GEMM of a mixture-of-experts layer for N > 1 tokens: k_experts_route in
// front of it (which row of the GEMM is which (token, slot), one expert per tile of 64 rows), k_experts_combine behind it.  DESIGN.md 4.18.
//
// k_experts_route: a stable counting sort of the N x S flat slots f = n S + s by expert, on the device, into POSITIONS: experts in
// increasing id, every expert's segment starting on a multiple of 64 positions (a tile of the grouped GEMM has one expert), increasing f
// inside a segment.  The result is a pure function of ids: no global atomic decides an order.
//   split    ONE workgroup of 16 waves; wave w owns the contiguous run [w run, (w + 1) run) of flat slots, run a multiple of 64.
//   count    cnt[w][e] in LDS (integer LDS atomics: a count has no order), 16 x E words.
//   scan     thread e turns column e into the exclusive prefix over the waves and keeps the expert's total; the totals' tile counts
//            ceil(c_e / 64) are scanned over the experts (Hillis-Steele in LDS, E <= 256); base[w][e] = 64 tile0[e] + prefix[w][e]: the
//            scan is expert-major and wave-minor with the padding to 64 folded in.
//   place    each wave walks its run 64 slots at a time: the lanes that hold the same id take consecutive positions from base[w][id] by
//            ballot and popcount (one round per distinct id of the 64), and the wave moves its base on.
//   tails    tile_expert[t] by a search of the tile prefix; src is -1 at every position behind an expert's last slot and in dead tiles;
//            pos is -1 for an empty slot (id outside [0, E)).  Every word of the three outputs is written exactly once.
// k_experts_combine: y[n][:] = sum_s gates[n][s] * C[pos[n S + s]][:], slot order, acc = fadd_rn(acc, fmul_rn(g, c)) from 0: one 16-byte
// load per slot and one store per four outputs, no atomics.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>

#include "tmac_kernels.h"

namespace tmac {

constexpr int ROUTE_NWV = 16, ROUTE_FT = 64 * ROUTE_NWV;
constexpr int ROUTE_MAX_T = EXPERTS_ROWS_MAX_NS / 64 + EXPERTS_ROWS_MAX_E;

__global__ __launch_bounds__(ROUTE_FT) void k_experts_route(const int32_t* __restrict__ ids, int NS, int E, int T_max, int32_t* __restrict__ tile_expert,
                                                            int32_t* __restrict__ src, int32_t* __restrict__ pos) {
    __shared__ int cnt[ROUTE_NWV * EXPERTS_ROWS_MAX_E];   // [wave][E]: counts, then bases
    __shared__ int total[EXPERTS_ROWS_MAX_E];             // slots of expert e
    __shared__ int tiles[2][EXPERTS_ROWS_MAX_E];          // the inclusive scan of ceil(total / 64), ping-pong
    const int tid = threadIdx.x, w = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int run = ((NS + ROUTE_FT - 1) / ROUTE_FT) * 64;                 // flat slots of a wave: whole 64s
    const int f_lo = w * run, f_hi = min(f_lo + run, NS);

    for (int i = tid; i < ROUTE_NWV * E; i += ROUTE_FT) cnt[i] = 0;
    __syncthreads();
    // ---- count -----------------------------------------------------------------------------------------------------------------
    for (int f0 = f_lo; f0 < f_hi; f0 += 64) {
        const int f = f0 + lane;
        const uint32_t id = f < f_hi ? (uint32_t)ids[f] : 0xffffffffu;
        if (id < (uint32_t)E) atomicAdd(&cnt[w * E + (int)id], 1);
    }
    __syncthreads();
    // ---- scan: over the waves of an expert (thread e), then over the experts' tile counts ------------------------------------------
    int my_total = 0;
    if (tid < E) {
        for (int ww = 0; ww < ROUTE_NWV; ++ww) {
            const int c = cnt[ww * E + tid];
            cnt[ww * E + tid] = my_total;
            my_total += c;
        }
        total[tid] = my_total;
        tiles[0][tid] = (my_total + 63) >> 6;
    }
    __syncthreads();
    int cur = 0;
    for (int d = 1; d < E; d <<= 1) {                                       // (uniform trip count: E is an argument)
        if (tid < E) tiles[cur ^ 1][tid] = tiles[cur][tid] + (tid >= d ? tiles[cur][tid - d] : 0);
        cur ^= 1;
        __syncthreads();
    }
    const int* tincl = tiles[cur];                                          // tiles of experts 0 .. e
    if (tid < E) {
        const int seg0 = 64 * (tincl[tid] - ((my_total + 63) >> 6));
        for (int ww = 0; ww < ROUTE_NWV; ++ww) cnt[ww * E + tid] += seg0;
    }
    __syncthreads();
    // ---- place: this wave's run, 64 slots at a time ----------------------------------------------------------------------------
    volatile int* wcnt = cnt + w * E;      // this wave's row: no other wave touches it; one lane writes what all 64 read next (volatile)
    for (int f0 = f_lo; f0 < f_hi; f0 += 64) {
        const int f = f0 + lane;
        const uint32_t id = f < f_hi ? (uint32_t)ids[f] : 0xffffffffu;
        bool todo = id < (uint32_t)E;
        int p = -1;
        unsigned long long left = __ballot(todo);
        while (left) {                                                      // one round per distinct id among the 64
            const int lead = __builtin_amdgcn_readfirstlane((int)__builtin_ctzll(left));
            const int e = __builtin_amdgcn_readlane((int)id, lead);
            const unsigned long long same = __ballot(todo && (int)id == e);
            const int base = wcnt[e];
            if (todo && (int)id == e) {
                p = base + __popcll(same & ((1ull << lane) - 1ull));
                todo = false;
            }
            if (lane == lead) wcnt[e] = base + __popcll(same);
            left &= ~same;
        }
        if (f < f_hi) {
            pos[f] = p;
            if (p >= 0) src[p] = f;
        }
    }
    // ---- tails: the tiles' experts, and -1 wherever no slot landed ----------------------------------------------------------------
    const int t_used = tincl[E - 1];
    for (int i = tid; i < 64 * T_max; i += ROUTE_FT) {
        const int t = i >> 6;
        int e = -1;
        if (t < t_used) {                                                   // the first expert whose inclusive tile count passes t
            int lo = 0, hi = E - 1;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (tincl[mid] > t) hi = mid; else lo = mid + 1;
            }
            e = lo;
        }
        if ((i & 63) == 0) tile_expert[t] = e;
        if (e < 0) src[i] = -1;
        else if (i - 64 * (tincl[e] - ((total[e] + 63) >> 6)) >= total[e]) src[i] = -1;
    }
}

hipError_t launch_experts_route(const int32_t* ids, int NS, int E, int T_max, int32_t* tile_expert, int32_t* src, int32_t* pos, hipStream_t st) {
    if (!ids || !tile_expert || !src || !pos || NS < 1 || NS > EXPERTS_ROWS_MAX_NS || E < 1 || E > EXPERTS_ROWS_MAX_E) return hipErrorInvalidValue;
    if (T_max < NS / 64 + (E < NS ? E : NS) || T_max > ROUTE_MAX_T) return hipErrorInvalidValue;     // (fewer tiles than the ids may need)
    hipLaunchKernelGGL(k_experts_route, dim3(1), dim3(ROUTE_FT), 0, st, ids, NS, E, T_max, tile_expert, src, pos);
    return hipGetLastError();
}

// thread = (token n = blockIdx.y, four outputs)
template <bool F16>
__global__ __launch_bounds__(256) void k_experts_combine(const float* __restrict__ C, const int32_t* __restrict__ pos, const float* __restrict__ gates,
                                                         int S, int Mw, int P, void* __restrict__ y) {
    const int n = blockIdx.y, o = 4 * (blockIdx.x * 256 + threadIdx.x);
    if (o >= Mw) return;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int s = 0; s < S; ++s) {
        const int p = pos[n * S + s];
        if ((uint32_t)p >= (uint32_t)P) continue;                           // an empty slot adds nothing
        const float g = gates[n * S + s];
        const float4 c = *reinterpret_cast<const float4*>(C + (size_t)p * Mw + o);
        acc.x = __fadd_rn(acc.x, __fmul_rn(g, c.x)); acc.y = __fadd_rn(acc.y, __fmul_rn(g, c.y));
        acc.z = __fadd_rn(acc.z, __fmul_rn(g, c.z)); acc.w = __fadd_rn(acc.w, __fmul_rn(g, c.w));
    }
    if constexpr (F16) {
        const __half2 h0 = __floats2half2_rn(acc.x, acc.y), h1 = __floats2half2_rn(acc.z, acc.w);
        *reinterpret_cast<uint2*>(reinterpret_cast<__half*>(y) + (size_t)n * Mw + o) =
            make_uint2(*reinterpret_cast<const uint32_t*>(&h0), *reinterpret_cast<const uint32_t*>(&h1));
    } else {
        *reinterpret_cast<float4*>(reinterpret_cast<float*>(y) + (size_t)n * Mw + o) = acc;
    }
}

hipError_t launch_experts_combine(const float* C, const int32_t* pos, const float* gates, int N, int S, int Mw, int P, void* y, int out_f16, hipStream_t st) {
    if (!C || !pos || !gates || !y || N < 1 || N > 65535 || S < 1 || S > EXPERTS_MAX_SLOTS || Mw < 4 || Mw % 4 != 0 || P < 64) return hipErrorInvalidValue;
    const dim3 g((Mw / 4 + 255) / 256, N), b(256);
    if (out_f16) hipLaunchKernelGGL(k_experts_combine<true>, g, b, 0, st, C, pos, gates, S, Mw, P, y);
    else hipLaunchKernelGGL(k_experts_combine<false>, g, b, 0, st, C, pos, gates, S, Mw, P, y);
    return hipGetLastError();
}

}  // namespace tmac
