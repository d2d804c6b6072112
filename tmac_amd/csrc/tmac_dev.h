// tmac_dev.h — device-only scalar and cross-lane helpers, one copy for every .hip of the library (tmac_core.h is also compiled by
// g++ for the CPU emulation, so nothing that needs hipcc lives there).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>

namespace tmac {

template <typename T> __device__ __forceinline__ float to_f32(T v);
template <> __device__ __forceinline__ float to_f32<float>(float v) { return v; }
template <> __device__ __forceinline__ float to_f32<__half>(__half v) { return __half2float(v); }
template <typename T> __device__ __forceinline__ T from_f32(float v);
template <> __device__ __forceinline__ float from_f32<float>(float v) { return v; }
template <> __device__ __forceinline__ __half from_f32<__half>(float v) { return __float2half_rn(v); }

// weight of bit-plane p in the plane combine (qgemm.py:192-206)
__device__ __forceinline__ float alpha_of(int p) { return p == 0 ? 0.5f : (p == 1 ? 1.0f : (p == 2 ? 2.0f : 4.0f)); }

// element i of an fp16 / fp32 scale array, element i of an fp16 / fp32 output
__device__ __forceinline__ float ld_scale(const void* p, int f16, size_t i) {
    return f16 ? __half2float(reinterpret_cast<const __half*>(p)[i]) : reinterpret_cast<const float*>(p)[i];
}
__device__ __forceinline__ void st_out(void* C, int f16, size_t i, float v) {
    if (f16) reinterpret_cast<__half*>(C)[i] = __float2half_rn(v);
    else reinterpret_cast<float*>(C)[i] = v;
}

// cvtps_epi32(round_ps(x)) + packs_epi32 + packs_epi16 (lut_ctor.cc:169-177): RNE then saturate
__device__ __forceinline__ int rne_sat_int8(float x) {
    const float r = rintf(x);
    int i = (r >= -2147483648.0f && r < 2147483648.0f) ? (int)r : INT32_MIN;
    return max(-128, min(127, i));
}

// Cross-lane moves as DPP modifiers (no LDS round trip, unlike __shfl_xor -> ds_bpermute_b32).
//   quad_perm [1,0,3,2] = 0xB1 (lane^1)   quad_perm [2,3,0,1] = 0x4E (lane^2)
//   row_shl:n = 0x100+n (lane i reads lane i+n of its 16-lane row)   row_ror:n = 0x120+n
//   row_half_mirror = 0x141 (i -> 7-i within 8)   row_mirror = 0x140 (i -> 15-i within 16)
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_u(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, false);
}

// value of lane ^ 16 / lane ^ 32 combined with the lane's own, on the VALU: gfx950's v_permlane16_swap / v_permlane32_swap exchange rows of 16
// (halves of 32) lanes between two registers; fed the same value twice they return {own | partner} and {partner | own} halves, whose sum
// (max) is what `x op __shfl_xor(x, 16 | 32)` computes -- bit for bit (the operations are commutative) -- without the ds_bpermute round trip
// through the LDS crossbar (two in a row in front of every reduction barrier of k_gemv_quad and k_decode_chain).  A/B knob: -DTMAC_SWAP_REDUCE=0.
#ifndef TMAC_SWAP_REDUCE
#define TMAC_SWAP_REDUCE 1
#endif
template <int W> __device__ __forceinline__ void q_swap_pair(uint32_t x, uint32_t& a0, uint32_t& a1) {
    if constexpr (W == 16) { const auto r = __builtin_amdgcn_permlane16_swap(x, x, false, false); a0 = r[0]; a1 = r[1]; }
    else { const auto r = __builtin_amdgcn_permlane32_swap(x, x, false, false); a0 = r[0]; a1 = r[1]; }
}
__device__ __forceinline__ float q_xor_add_f(float x) {          // x + x(lane ^ 16), then + (lane ^ 32)
#if TMAC_SWAP_REDUCE
    uint32_t a0, a1;
    q_swap_pair<16>(__float_as_uint(x), a0, a1); x = __fadd_rn(__uint_as_float(a0), __uint_as_float(a1));
    q_swap_pair<32>(__float_as_uint(x), a0, a1); x = __fadd_rn(__uint_as_float(a0), __uint_as_float(a1));
    return x;
#else
    x = __fadd_rn(x, __shfl_xor(x, 16, 64));
    return __fadd_rn(x, __shfl_xor(x, 32, 64));
#endif
}
__device__ __forceinline__ uint32_t q_xor_add_u(uint32_t x) {
#if TMAC_SWAP_REDUCE
    uint32_t a0, a1;
    q_swap_pair<16>(x, a0, a1); x = a0 + a1;
    q_swap_pair<32>(x, a0, a1); x = a0 + a1;
    return x;
#else
    x += (uint32_t)__shfl_xor((int)x, 16, 64);
    return x + (uint32_t)__shfl_xor((int)x, 32, 64);
#endif
}
__device__ __forceinline__ float q_xor_max_f(float x) {
#if TMAC_SWAP_REDUCE
    uint32_t a0, a1;
    q_swap_pair<16>(__float_as_uint(x), a0, a1); x = fmaxf(__uint_as_float(a0), __uint_as_float(a1));
    q_swap_pair<32>(__float_as_uint(x), a0, a1); x = fmaxf(__uint_as_float(a0), __uint_as_float(a1));
    return x;
#else
    x = fmaxf(x, __shfl_xor(x, 16, 64));
    return fmaxf(x, __shfl_xor(x, 32, 64));
#endif
}

// A lane's weight fragment of one (row block, step): the weight dwords and the raw scale / zero-point words of its rows, fetched WITH
// the weights (converted at use: converting at load time would stall on the load)
template <int BITS>
struct WFrag {
    uint32_t wd[8 * BITS / 2];
    uint32_t sraw[4];
};
// scale (which = 0) or zero point (which = 1) of row i (0/1) from the raw words
template <bool ZP>
__device__ __forceinline__ float frag_scale(const uint32_t (&sraw)[4], int f16, int i, int which) {
    const int e = i * (ZP ? 2 : 1) + which;          // element index within the lane's 2*per values
    if (f16) {
        const uint32_t wv = sraw[e >> 1];
        return __half2float(__ushort_as_half((unsigned short)((e & 1) ? (wv >> 16) : (wv & 0xffff))));
    }
    return __uint_as_float(sraw[e]);
}

}  // namespace tmac
