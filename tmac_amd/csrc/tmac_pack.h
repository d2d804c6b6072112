// tmac_pack.h — index and nibble arithmetic of the weight packers (tmac_pack.hip), for host and device.
//
// GPTQ tensors or plain codes -> the reference's bit-interleaved blob (python/t_mac/weights.py:57-87; closed form in
// tmac_amd/weights.py).  Everything here is a pure function of integers: tests/cpp/pack_main.cc compiles this header with plain g++
// and packs whole matrices through it, byte for byte against tmac_amd/weights.py:preprocess_weights (tests/test_pack_cpu.py); the
// kernels call the same functions.  The one piece of floating point: the BitNet absmean rule (master weights -> ternary levels), shared
// the same way with tests/cpp/pack_dense_main.cc.  The packed ternary format of BitNet checkpoints (four weight rows per byte) is integers
// again: tests/cpp/pack_ternary_main.cc.  Floating point once more: per-group round to nearest of dense masters to W1 - W4 codes (scale, zero
// code, code, the fp16 rounding of the scale), shared with tests/cpp/pack_rtn_main.cc.  Integers again: the AutoAWQ field rule and its plane
// extraction (eight weight rows per word along the output axis), shared with tests/cpp/pack_awq_main.cc.
//
//   M-space row     r    = (o / 8) * 8 * bits + p * 8 + o % 8                                (o: weight row, p: bit plane)
//   nibble(r, t)         = sum_ig bit_p(w[o][4 t + ig]) << ig
//   byte(r, t)           = tile * (bm / 2 * K / 4) + ((t / kfactor) * (bm / 32) + rr / 32) * kfactor * 16 + (t % kfactor) * 16 + rr % 16
//                          tile = r / bm, rr = r % bm;  low nibble for rr % 32 < 16, high otherwise
//   scale(o, sg, which)  = ((tile * SG + sg) * (rpt / 8) + ol / 8) * (8 | 16) + which * 8 + ol % 8,   rpt = bm / bits, tile = o / rpt, ol = o % rpt
//                          (which: 0 scale, 1 zero; 16 per octet with zero points)
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_fp16.h>
#define TMAC_PACK_HD __host__ __device__ __forceinline__
#else
#define TMAC_PACK_HD inline
#endif

namespace tmac_pack {

// M-space row of (weight row o, plane p), and its inverse
TMAC_PACK_HD int mrow(int o, int p, int bits) { return (o / 8) * 8 * bits + p * 8 + (o % 8); }
TMAC_PACK_HD int mrow_weight_row(int r, int bits) { return (r / (8 * bits)) * 8 + r % 8; }
TMAC_PACK_HD int mrow_plane(int r, int bits) { return (r % (8 * bits)) / 8; }

// byte of the blob that holds nibble (r, t); T = K / 4
TMAC_PACK_HD size_t blob_byte(int r, int t, int bm, int kfactor, int T) {
    const int tile = r / bm, rr = r % bm;
    return (size_t)tile * ((size_t)(bm / 2) * T) + ((size_t)(t / kfactor) * (bm / 32) + rr / 32) * ((size_t)kfactor * 16) +
           (size_t)(t % kfactor) * 16 + rr % 16;
}
TMAC_PACK_HD bool blob_high(int r, int bm) { return (r % bm) % 32 >= 16; }
// The 16 bytes that hold table t of the 32 M-space rows [32 g, 32 g + 32): byte j = nibble(32 g + j) | nibble(32 g + 16 + j) << 4.
// bm is a multiple of 32, so a group never straddles a tile.
TMAC_PACK_HD size_t blob_unit(int g, int t, int bm, int kfactor, int T) { return blob_byte(32 * g, t, bm, kfactor, T); }

// element of scales_ref that holds the scale (which = 0) or zero (which = 1) of (weight row o, scale group sg)
TMAC_PACK_HD size_t scale_index(int o, int sg, int which, int bm, int bits, int SG, int zero_point) {
    const int rpt = bm / bits, tile = o / rpt, ol = o % rpt;
    return (((size_t)tile * SG + sg) * (rpt / 8) + ol / 8) * (zero_point ? 16 : 8) + (size_t)which * 8 + ol % 8;
}

// Plain codes: the nibble of plane p from the four codes of one table (codes k = 4 t .. 4 t + 3 in bytes 0 .. 3 of `four`).  Bits of a
// code above `bits` are never looked at.
TMAC_PACK_HD uint32_t codes_nibble(uint32_t four, int p) {
    return ((four >> p) & 1u) | (((four >> (8 + p)) & 1u) << 1) | (((four >> (16 + p)) & 1u) << 2) | (((four >> (24 + p)) & 1u) << 3);
}

// GPTQ: one qweight word holds 32 / bits codes of consecutive k, lowest field first -- 8 / bits tables.  Plane p of the word: bit f of
// the result is bit p of field f, i.e. the nibbles of the word's tables, lowest table first (32 / bits valid bits).
TMAC_PACK_HD uint32_t gptq_plane(uint32_t word, int p, int bits) {
    if (bits == 1) return word;
    uint32_t out = 0;
    const int n = 32 / bits;
    for (int f = 0; f < n; ++f) out |= ((word >> (f * bits + p)) & 1u) << f;
    return out;
}
// field i of a packed row (qzeros: column m of row sg is field m % (32 / bits) of word m * bits / 32)
TMAC_PACK_HD uint32_t gptq_field(uint32_t word, int i, int bits) { return (word >> (i * bits)) & ((1u << bits) - 1u); }

// Act-order (packing through a K permutation, tmac_kperm.h): table t of the packed matrix takes its four codes from the SOURCE columns
// perm[4 t .. 4 t + 3].  GPTQ: the code of source column k sits in qweight word row k / (32 / bits) at bit (k % (32 / bits)) * bits.
TMAC_PACK_HD int gptq_word_row(int k, int bits) { return k / (32 / bits); }
TMAC_PACK_HD uint32_t gptq_code(uint32_t word, int k, int bits) { return gptq_field(word, k % (32 / bits), bits); }
// four gathered codes -> the `four` codes_nibble takes (code i in byte i)
TMAC_PACK_HD uint32_t codes_four(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3) { return c0 | (c1 << 8) | (c2 << 16) | (c3 << 24); }

// T-MAC's zero as a multiplier of the scale: z + (v1 ? 1 : 0) - 2^(bits-1), exact in fp16 and fp32 (convert.py:unpack_gptq; AutoGPTQ v1
// stores z - 1).  The zero itself is multiplier * scale, rounded ONCE to the scales' dtype: the fp32 product of an fp16 scale and this
// small integer is exact, so one conversion to fp16 gives numpy's fp16 product (overflow to infinity included).
TMAC_PACK_HD float gptq_zero_multiplier(uint32_t z, int v1, int bits) { return (float)((int)z + (v1 ? 1 : 0) - (1 << (bits - 1))); }

// ---- AutoAWQ (WQLinear_GEMM, 4 bits) -------------------------------------------------------------------------------------
// qweight int32 [K][Mw / 8] packs along the OUTPUT axis: word (k, c) holds the codes of the eight weight rows 8 c .. 8 c + 7 at column k,
// interleaved -- field i (bits 4 i .. 4 i + 3) belongs to row 8 c + ORDER[i], ORDER = (0, 2, 4, 6, 1, 3, 5, 7); row 8 c + j sits in field
// INV[j], INV = (0, 4, 1, 5, 2, 6, 3, 7).  qzeros int32 [K / gs][Mw / 8] the same way.  Known answer: 0x76543210 gives rows 8 c .. 8 c + 7
// the codes 0, 4, 1, 5, 2, 6, 3, 7.  The codes are T-MAC's as they stand; the stored zero is z itself (no + 1): gptq_zero_multiplier(z, 0, 4).
TMAC_PACK_HD int awq_row_of_field(int i) { return (i % 4) * 2 + i / 4; }        // ORDER
TMAC_PACK_HD int awq_field_of_row(int j) { return (j % 2) * 4 + j / 2; }        // INV
TMAC_PACK_HD uint32_t awq_code(uint32_t word, int row_in_octet) { return (word >> (4 * awq_field_of_row(row_in_octet))) & 15u; }
// Plane extraction.  The four words of one octet of weight rows at the four columns of ONE table (k = 4 t .. 4 t + 3) -> the eight
// nibbles of plane p, in FIELD order: bit ig of nibble i is bit p of field i of word ig, so the nibble of row j of the octet is
// awq_code(result, j) -- eight rows for four shift-and-mask steps.
TMAC_PACK_HD uint32_t awq_plane_nibbles(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, int p) {
    const uint32_t m = 0x11111111u;
    return ((w0 >> p) & m) | (((w1 >> p) & m) << 1) | (((w2 >> p) & m) << 2) | (((w3 >> p) & m) << 3);
}
// lo / hi: awq_plane_nibbles of tables 2 tp and 2 tp + 1 -> the byte a packer's LDS image holds for (plane, row j of the octet, table pair
// tp): the nibble of table 2 tp in the low half, of table 2 tp + 1 in the high half
TMAC_PACK_HD uint32_t awq_plane_byte(uint32_t lo, uint32_t hi, int row_in_octet) { return awq_code(lo, row_in_octet) | (awq_code(hi, row_in_octet) << 4); }

// ---- BitNet b1.58: master weights -> ternary levels (the absmean rule) -----------------------------------------------
// A row block of R = Mw / m_groups rows has ONE scale:
//   gamma = fp32(sum |fp64(w)| / (R K))     the sum in fp64, in an order (Mw, K, m_groups) alone decide: absmean_chunks, k_absmean
//   s     = fmaxf(gamma, eps)               the unified scale the blob stores
//   level = absmean_level(w, 1 / s)         {-1, 0, 1} + 2: levels 1, 2, 3 of the 2-bit format, w_real = (level - 2) s; level 0 unused
// Every step is one correctly rounded fp32 operation, written the same for the device and for plain g++ (tests/cpp/pack_dense_main.cc);
// the conversions of fp16 and bf16 masters to fp32, and of |w| to fp64, are exact.
// Non-finite masters: an infinity makes gamma, and so s, +infinity and 1 / s zero -- every finite master of the block then quantises
// to 0 and the infinities themselves (inf * 0 is NaN) too; a NaN makes gamma NaN, which fmaxf drops: s = eps.  Neither changes an address.
enum { SRC_F32 = 0, SRC_F16 = 1, SRC_BF16 = 2 };       // tmac_src_dtype_t

// fp64 reduction, stage A: a workgroup sums one chunk of ABSMEAN_CHUNK consecutive elements of a row block (the block's last chunk may be
// short); stage B adds a block's chunk sums in index order.  A function of the block's element count alone.
constexpr int ABSMEAN_THREADS = 256;
constexpr int ABSMEAN_VEC = 4;                          // elements per load: 16 bytes of fp32, 8 bytes of fp16 / bf16
constexpr int ABSMEAN_STEPS = 16;                       // loads per thread
constexpr size_t ABSMEAN_CHUNK = (size_t)ABSMEAN_THREADS * ABSMEAN_VEC * ABSMEAN_STEPS;
TMAC_PACK_HD size_t absmean_chunks(size_t block_elems) { return (block_elems + ABSMEAN_CHUNK - 1) / ABSMEAN_CHUNK; }

TMAC_PACK_HD float bf16_bits_to_f32(uint16_t h) {
    const uint32_t x = (uint32_t)h << 16;
    float f;
    __builtin_memcpy(&f, &x, 4);
    return f;
}
// sum: the block's fp64 sum of |w|; count: its R * K elements
TMAC_PACK_HD float absmean_scale(double sum, double count, float eps) { return fmaxf((float)(sum / count), eps); }
TMAC_PACK_HD float absmean_inv(float s) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fdiv_rn(1.0f, s);
#else
    return 1.0f / s;
#endif
}
TMAC_PACK_HD uint32_t absmean_level(float w, float inv) {
#if defined(__HIP_DEVICE_COMPILE__)
    const float q = __fmul_rn(w, inv);
#else
    const float q = w * inv;
#endif
    // round half to even (rintf in the default rounding mode), clamp to [-1, 1].  A NaN -- a NaN master, or an infinite one times a zero
    // inverse -- is 0: said here, because fmaxf / fminf would turn it into -1.
    const float t = q != q ? 0.0f : fminf(fmaxf(rintf(q), -1.0f), 1.0f);
    return (uint32_t)((int)t + 2);
}
// four masters of one table -> the `four` codes_nibble takes
TMAC_PACK_HD uint32_t absmean_four(float w0, float w1, float w2, float w3, float inv) {
    return codes_four(absmean_level(w0, inv), absmean_level(w1, inv), absmean_level(w2, inv), absmean_level(w3, inv));
}

// ---- BitNet b1.58: packed ternary checkpoints (the Hugging Face BitNet quantiser, offline mode) -----------------------
// packed uint8 [R4][K], R4 = Mw / 4: weight row o lives in packed row o % R4, in the 2-bit field o / R4 at bit 2 (o / R4) -- the four row
// blocks of the matrix share a byte.  The stored field is v = t + 1 with t in {-1, 0, 1}; the 2-bit level of the blob is t + 2 = v + 1
// (levels 1, 2, 3 as above).  v = 3 occurs in no well-formed file: it has no level, is packed as level 3 (t = 2 clamped to 1) and counted.
TMAC_PACK_HD int ternary_packed_row(int o, int R4) { return o % R4; }
TMAC_PACK_HD int ternary_field(int o, int R4) { return o / R4; }
TMAC_PACK_HD uint32_t ternary_level(uint32_t v) { return v >= 3u ? 3u : v + 1u; }
// The four packed bytes of one table (columns 4 t .. 4 t + 3 of a packed row, column i in byte i of `bytes`) and a field index -> the
// `four` codes_nibble takes for the weight row that owns the field; *invalid: how many of the four fields were 3.
TMAC_PACK_HD uint32_t ternary_four(uint32_t bytes, int field, int* invalid) {
    const uint32_t v = (bytes >> (2 * field)) & 0x03030303u;
    const uint32_t three = v & (v >> 1) & 0x01010101u;      // 1 in the bytes whose field is 3
    *invalid = __builtin_popcount(three);
    return v + 0x01010101u - three;                         // ternary_level of each byte: no carry leaves a byte
}

// ---- dense master weights -> W1 - W4 codes with per-group scales: round to nearest -----------------------------------
// GPTQ's quantiser without the error search (Quantizer.find_params with mse = False, then quantize).  For weight row o and group sg of gs
// consecutive k, maxq = 2^bits - 1, every step one correctly rounded fp32 operation:
//   lo = min(min_k w, 0), hi = max(max_k w, 0)              exact: the order of the reduction cannot matter
//   symmetric (no zero points):  hi = max(|lo|, hi), lo = -hi, zq = 2^(bits-1)
//   scale = (hi - lo) / maxq;   lo == hi == 0, or scale below the smallest normal fp32: lo = -1, hi = +1 (GPTQ's all-zero group)
//   scale_f16: scale = fp16(scale) -- the scale that divides is the scale the handle stores
//   asymmetric:  zq = rint(-lo / scale)                     ties to even; no clamp, as in GPTQ
//   code = clamp(rint(w / scale) + zq, 0, maxq);   T-MAC's zero = (zq - 2^(bits-1)) * scale, w_real = (code - 2^(bits-1)) * scale - zero
// A group is INVALID when a master of it is not finite or its scale is 0 or not finite (an fp16 scale that under- or overflowed): it gets
// the parameters of the all-zero group and is counted.  Parameters live in fp32 [Mw][SG] arrays, SG = K / gs: rtn_param_index.
TMAC_PACK_HD float round_to_f16(float v);
TMAC_PACK_HD size_t rtn_param_index(int o, int sg, int SG) { return (size_t)o * SG + sg; }
TMAC_PACK_HD float rtn_div(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fdiv_rn(a, b);
#else
    return a / b;
#endif
}
TMAC_PACK_HD bool rtn_finite(float v) { return v - v == 0.0f; }        // false for an infinity and for a NaN
// lo <= 0 <= hi: the group's minimum and maximum, each already taken with 0 (fminf / fmaxf: a NaN master is dropped); finite: every master
// of the group is.  Returns whether the group is valid; *scale and *zq of an invalid group are those of the all-zero group.
TMAC_PACK_HD bool rtn_scale_zq(float lo, float hi, bool finite, int bits, int zero_point, int scale_f16, float* scale, float* zq) {
    const float maxq = (float)((1 << bits) - 1);
    if (!finite) lo = hi = 0.0f;
    if (!zero_point) {
        hi = fmaxf(fabsf(lo), hi);
        lo = -hi;
    }
    if (lo == 0.0f && hi == 0.0f) { lo = -1.0f; hi = 1.0f; }
    float s = rtn_div(hi - lo, maxq);
    if (s < 1.17549435e-38f) { lo = -1.0f; hi = 1.0f; s = rtn_div(2.0f, maxq); }
    if (scale_f16) s = round_to_f16(s);
    const bool ok = finite && s != 0.0f && rtn_finite(s);
    if (!ok) {
        lo = -1.0f; hi = 1.0f;
        s = rtn_div(2.0f, maxq);
        if (scale_f16) s = round_to_f16(s);
    }
    *scale = s;
    *zq = zero_point ? rintf(rtn_div(-lo, s)) + 0.0f : (float)(1 << (bits - 1));      // + 0: -0 (lo = +0) becomes +0
    return ok;
}
// a NaN quotient -- a NaN master; its group is invalid -- gives code 0: fmaxf drops it
TMAC_PACK_HD uint32_t rtn_code(float w, float scale, float zq, int bits) {
    return (uint32_t)fminf(fmaxf(rintf(rtn_div(w, scale)) + zq, 0.0f), (float)((1 << bits) - 1));
}
TMAC_PACK_HD float rtn_zero(float scale, float zq, int bits) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fmul_rn(zq - (float)(1 << (bits - 1)), scale);
#else
    return (zq - (float)(1 << (bits - 1))) * scale;
#endif
}
// four masters of one table -> the `four` codes_nibble takes
TMAC_PACK_HD uint32_t rtn_four(float w0, float w1, float w2, float w3, float scale, float zq, int bits) {
    return codes_four(rtn_code(w0, scale, zq, bits), rtn_code(w1, scale, zq, bits), rtn_code(w2, scale, zq, bits), rtn_code(w3, scale, zq, bits));
}

#if defined(__HIPCC__)
TMAC_PACK_HD float round_to_f16(float v) { return __half2float(__float2half_rn(v)); }
#else
// IEEE binary16 bits of v, round to nearest even (subnormals, overflow to infinity, NaN), and back: what numpy's float16 does
inline uint16_t f32_to_f16_bits(float v) {
    uint32_t x;
    __builtin_memcpy(&x, &v, 4);
    const uint32_t sign = (x >> 16) & 0x8000u, mag = x & 0x7fffffffu;
    if (mag >= 0x7f800000u) return (uint16_t)(sign | 0x7c00u | (mag > 0x7f800000u ? 0x200u : 0u));
    if (mag >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);                 // >= 65520 rounds to infinity
    if (mag < 0x33000001u) return (uint16_t)sign;                             // <= 2^-25 rounds to zero
    const int e = (int)(mag >> 23) - 127;
    uint32_t m = (mag & 0x7fffffu) | 0x800000u;
    const int shift = e < -14 ? 13 + (-14 - e) : 13;                          // subnormal results lose more bits
    const uint32_t rest = m & ((1u << shift) - 1u), half = 1u << (shift - 1);
    m >>= shift;
    if (rest > half || (rest == half && (m & 1u))) ++m;
    // normal: m has the hidden bit at 0x400, adding (e + 14) << 10 lets a carry out of the mantissa bump the exponent
    const uint32_t h = e < -14 ? m : (uint32_t)((e + 14) << 10) + m;
    return (uint16_t)(sign | h);
}
inline float f16_bits_to_f32(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3ffu;
    float mag;
    if (e == 31) {
        const uint32_t x = 0x7f800000u | (m << 13);
        __builtin_memcpy(&mag, &x, 4);
    } else if (e == 0) {
        mag = (float)m * (1.0f / 16777216.0f);                                 // m * 2^-24
    } else {
        const uint32_t x = ((e + 112u) << 23) | (m << 13);
        __builtin_memcpy(&mag, &x, 4);
    }
    uint32_t x;
    __builtin_memcpy(&x, &mag, 4);
    x |= sign;
    __builtin_memcpy(&mag, &x, 4);
    return mag;
}
inline float round_to_f16(float v) { return f16_bits_to_f32(f32_to_f16_bits(v)); }
#endif

}  // namespace tmac_pack
