// tmac_pack.hip — device-side packing: GPTQ tensors or plain codes -> the reference's bit-interleaved blob (A_ref, scales_ref), the
// input of weight registration.  A pure permutation of bits; index arithmetic in tmac_pack.h (shared with the host test).
//
// Weights: one workgroup per tile of 64 weight rows x 64 tables (256 values of K).
//   stage 1  every input word of the tile is read once, coalesced along the input's fast axis (GPTQ [k][m]: 16 bytes per lane along m;
//            codes [m][k]: 4 bytes per lane along k), split into bit planes and written to LDS as nibbles: row (plane, weight row), two
//            tables per byte.  GPTQ: the 8 / bits tables of a word are contiguous bits of the plane word -- one LDS store per plane.
//            Codes: the 8 lanes that hold 8 consecutive tables OR their nibbles together (3 xor shuffles), one 32-bit store per plane.
//   stage 2  one thread per (group of 32 M-space rows, pair of tables): 32 LDS bytes -> the two 16-byte units of the blob, each written
//            by exactly this thread.  Lanes walk the tables, so a wave's stores run along the blob's kfactor * 16-byte runs.
// Tails (Mw not a multiple of 64, K / 4 not a multiple of 64) are guarded on both sides: nothing outside the inputs is loaded, nothing
// outside the blob is stored.  No atomics, no read-modify-write.
// Scales: one thread per (scale group, 8 weight rows) writes the 8 scales (and 8 zeros) of that octet as 16-byte stores.
// BitNet master weights (fp32 / fp16 / bf16 [Mw][K]): the scale of each row block by a two-stage fp64 reduction (k_absmean,
// k_absmean_scales), then the codes kernel with a stage 1 that quantises four masters per lane (k_pack_dense_weights).
// BitNet packed ternary weights (uint8 [Mw / 4][K], four weight rows per byte): the codes kernel with a stage 1 that extracts a field
// (k_pack_ternary_weights), or, where no group of 32 M-space rows straddles two fields, one load of every byte feeding four output tiles
// (k_pack_ternary_weights_x4); fields without a ternary level are counted.
// Dense master weights to W1 - W4 with per-group scales (round to nearest): the scale and zero code of every (row, group) from its minimum
// and maximum (k_rtn_params; groups that cannot be quantised are counted), then the codes kernel with a stage 1 that quantises four masters
// per lane under them (k_pack_rtn_weights) and the codes form's scales kernel.
// AutoAWQ GEMM tensors (qweight int32 [K][Mw / 8], eight weight rows per word along the output axis, interleaved): a stage 1 that owns
// (octets of weight rows, a pair of tables) and turns eight words of consecutive k into the LDS bytes of eight rows (k_pack_awq_weights),
// several 64-row output tiles per workgroup, and the GPTQ scales kernel with the zero taken from the interleaved field (k_pack_awq_scales).
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include "tmac_dev.h"
#include "tmac_kernels.h"
#include "tmac_pack.h"

namespace tmac {
namespace {

namespace pk = tmac_pack;

constexpr int PACK_ROWS = 64;              // weight rows per tile
constexpr int PACK_TABLES = 64;            // tables per tile
constexpr int PACK_THREADS = 256;
constexpr int PACK_STRIDE = PACK_TABLES / 2 + 4;   // bytes per LDS row: 9 words, consecutive rows fall on consecutive banks

// LDS row of (plane p, local weight row ol)
__device__ __forceinline__ int lds_row(int p, int ol) { return p * PACK_ROWS + ol; }

// stage 2, shared by every input form: the LDS tile `lds` holds the groups of 32 M-space rows [g0, g0 + GROUPS) of the matrix, of which
// those below g_end exist
template <int BITS>
__device__ __forceinline__ void pack_store_groups(const uint8_t* lds, uint8_t* __restrict__ A_out, int g0, int g_end, int T, int bm, int kfactor) {
    const int t0 = blockIdx.x * PACK_TABLES;
    constexpr int GROUPS = PACK_ROWS * BITS / 32;       // groups of 32 M-space rows per tile
    for (int item = threadIdx.x; item < GROUPS * (PACK_TABLES / 2); item += PACK_THREADS) {
        const int gl = item / (PACK_TABLES / 2), tp = item % (PACK_TABLES / 2);
        const int g = g0 + gl, t = t0 + 2 * tp;
        if (g >= g_end || t >= T) continue;
        uint32_t u0[4] = {0, 0, 0, 0}, u1[4] = {0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int rlo = gl * 32 + j, rhi = rlo + 16;
            const uint32_t lo = lds[lds_row(pk::mrow_plane(rlo, BITS), pk::mrow_weight_row(rlo, BITS)) * PACK_STRIDE + tp];
            const uint32_t hi = lds[lds_row(pk::mrow_plane(rhi, BITS), pk::mrow_weight_row(rhi, BITS)) * PACK_STRIDE + tp];
            u0[j / 4] |= ((lo & 15u) | ((hi & 15u) << 4)) << (8 * (j % 4));
            u1[j / 4] |= ((lo >> 4) | (hi & 0xf0u)) << (8 * (j % 4));
        }
        *reinterpret_cast<uint4*>(A_out + pk::blob_unit(g, t, bm, kfactor, T)) = make_uint4(u0[0], u0[1], u0[2], u0[3]);
        if (t + 1 < T) *reinterpret_cast<uint4*>(A_out + pk::blob_unit(g, t + 1, bm, kfactor, T)) = make_uint4(u1[0], u1[1], u1[2], u1[3]);
    }
}
// ... of the tile of weight rows blockIdx.y names
template <int BITS>
__device__ __forceinline__ void pack_store_tile(const uint8_t* lds, uint8_t* __restrict__ A_out, int Mw, int T, int bm, int kfactor) {
    // M is a multiple of 32 (bm is)
    pack_store_groups<BITS>(lds, A_out, blockIdx.y * (PACK_ROWS * BITS / 32), Mw * BITS / 32, T, bm, kfactor);
}

// GPTQ qweight int32 [K * BITS / 32][Mw]
template <int BITS>
__global__ __launch_bounds__(PACK_THREADS) void k_pack_gptq_weights(const uint32_t* __restrict__ qweight, uint8_t* __restrict__ A_out, int Mw,
                                                                    int K, int bm, int kfactor) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[PACK_ROWS * BITS * PACK_STRIDE];
    const int T = K / 4, KP = K / (32 / BITS);
    const int o0 = blockIdx.y * PACK_ROWS;
    constexpr int WORD_ROWS = PACK_TABLES * BITS / 8;       // qweight rows per tile: a word holds 8 / BITS tables
    const int kp0 = blockIdx.x * WORD_ROWS;
    for (int idx = threadIdx.x; idx < WORD_ROWS * (PACK_ROWS / 4); idx += PACK_THREADS) {
        const int kpl = idx / (PACK_ROWS / 4), mq = idx % (PACK_ROWS / 4);
        const int kp = kp0 + kpl, m = o0 + 4 * mq;
        uint4 w4 = make_uint4(0, 0, 0, 0);
        if (kp < KP && m < Mw) w4 = *reinterpret_cast<const uint4*>(qweight + (size_t)kp * Mw + m);   // Mw is a multiple of 8: whole quads
        const uint32_t w[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
#pragma unroll
            for (int p = 0; p < BITS; ++p) {
                const uint32_t v = pk::gptq_plane(w[c], p, BITS);
                uint8_t* dst = lds + lds_row(p, 4 * mq + c) * PACK_STRIDE + kpl * (4 / BITS);    // 8 / BITS tables = 4 / BITS bytes
                if (BITS == 1) *reinterpret_cast<uint32_t*>(dst) = v;
                else if (BITS == 2) *reinterpret_cast<uint16_t*>(dst) = (uint16_t)v;
                else *dst = (uint8_t)v;
            }
        }
    }
    __syncthreads();
    pack_store_tile<BITS>(lds, A_out, Mw, T, bm, kfactor);
}

// plain codes uint8 [Mw][K]
template <int BITS>
__global__ __launch_bounds__(PACK_THREADS) void k_pack_codes_weights(const uint8_t* __restrict__ codes, uint8_t* __restrict__ A_out, int Mw, int K,
                                                                     int bm, int kfactor) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[PACK_ROWS * BITS * PACK_STRIDE];
    const int T = K / 4;
    const int o0 = blockIdx.y * PACK_ROWS, t0 = blockIdx.x * PACK_TABLES;
    // a wave takes one weight row's 64 tables per step (256 contiguous bytes); every lane runs every step (the shuffles need them all)
    for (int idx = threadIdx.x; idx < PACK_ROWS * PACK_TABLES; idx += PACK_THREADS) {
        const int ol = idx / PACK_TABLES, tl = idx % PACK_TABLES;
        const int o = o0 + ol, t = t0 + tl;
        uint32_t four = 0;
        if (o < Mw && t < T) four = *reinterpret_cast<const uint32_t*>(codes + (size_t)o * K + 4 * (size_t)t);   // K is a multiple of 4
#pragma unroll
        for (int p = 0; p < BITS; ++p) {
            uint32_t v = pk::codes_nibble(four, p) << (4 * (tl % 8));
            v |= __shfl_xor(v, 1);
            v |= __shfl_xor(v, 2);
            v |= __shfl_xor(v, 4);
            if (tl % 8 == 0) *reinterpret_cast<uint32_t*>(lds + lds_row(p, ol) * PACK_STRIDE + tl / 2) = v;
        }
    }
    __syncthreads();
    pack_store_tile<BITS>(lds, A_out, Mw, T, bm, kfactor);
}

// ---- act-order: stage 1 through a K permutation (tmac_kperm.h) ----------------------------------------------------------------------
// Table t of the tile takes its four codes from the source columns perm[4 t .. 4 t + 3] (one 16-byte load: perm is [K], K a multiple of 4,
// 16-byte aligned).  Every perm value is < K (tmac_hip_kperm_from_gidx_dev refuses anything else), so the gathers stay inside the inputs;
// the guards on t and on the weight row are those of the plain kernels.  A thread takes a PAIR of tables and writes the byte that holds
// their two nibbles itself: no two threads share an LDS byte.  Stage 2 and the scale kernels are the plain ones (scales and zeros are in
// group order already).  The gather reads a whole qweight word (a whole codes byte) per code: 8 / bits times the plain traffic, once.
template <int BITS>
__global__ __launch_bounds__(PACK_THREADS) void k_pack_gptq_weights_perm(const uint32_t* __restrict__ qweight, const int32_t* __restrict__ perm,
                                                                         uint8_t* __restrict__ A_out, int Mw, int K, int bm, int kfactor) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[PACK_ROWS * BITS * PACK_STRIDE];
    const int T = K / 4;
    const int o0 = blockIdx.y * PACK_ROWS, t0 = blockIdx.x * PACK_TABLES;
    // consecutive threads take consecutive row quads of one table pair: the 16-byte loads of a source column run along m
    for (int idx = threadIdx.x; idx < (PACK_TABLES / 2) * (PACK_ROWS / 4); idx += PACK_THREADS) {
        const int tp = idx / (PACK_ROWS / 4), mq = idx % (PACK_ROWS / 4);
        const int m = o0 + 4 * mq;
        uint32_t nib[2][4][BITS];      // [table of the pair][row of the quad][plane]
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int t = t0 + 2 * tp + h;
            uint32_t code[4][4] = {};  // [row of the quad][column of the table]
            if (t < T && m < Mw) {
                const int4 src = *reinterpret_cast<const int4*>(perm + 4 * (size_t)t);
                const int k4[4] = {src.x, src.y, src.z, src.w};
#pragma unroll
                for (int ig = 0; ig < 4; ++ig) {
                    const uint4 w4 = *reinterpret_cast<const uint4*>(qweight + (size_t)pk::gptq_word_row(k4[ig], BITS) * Mw + m);   // Mw is a multiple of 8: whole quads
                    code[0][ig] = pk::gptq_code(w4.x, k4[ig], BITS); code[1][ig] = pk::gptq_code(w4.y, k4[ig], BITS);
                    code[2][ig] = pk::gptq_code(w4.z, k4[ig], BITS); code[3][ig] = pk::gptq_code(w4.w, k4[ig], BITS);
                }
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const uint32_t four = pk::codes_four(code[c][0], code[c][1], code[c][2], code[c][3]);
#pragma unroll
                for (int p = 0; p < BITS; ++p) nib[h][c][p] = pk::codes_nibble(four, p);
            }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int p = 0; p < BITS; ++p) lds[lds_row(p, 4 * mq + c) * PACK_STRIDE + tp] = (uint8_t)(nib[0][c][p] | (nib[1][c][p] << 4));
    }
    __syncthreads();
    pack_store_tile<BITS>(lds, A_out, Mw, T, bm, kfactor);
}

// plain codes uint8 [Mw][K]: one byte load per code; consecutive threads take consecutive table pairs of one weight row
template <int BITS>
__global__ __launch_bounds__(PACK_THREADS) void k_pack_codes_weights_perm(const uint8_t* __restrict__ codes, const int32_t* __restrict__ perm,
                                                                          uint8_t* __restrict__ A_out, int Mw, int K, int bm, int kfactor) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[PACK_ROWS * BITS * PACK_STRIDE];
    const int T = K / 4;
    const int o0 = blockIdx.y * PACK_ROWS, t0 = blockIdx.x * PACK_TABLES;
    for (int idx = threadIdx.x; idx < PACK_ROWS * (PACK_TABLES / 2); idx += PACK_THREADS) {
        const int ol = idx / (PACK_TABLES / 2), tp = idx % (PACK_TABLES / 2);
        const int o = o0 + ol;
        uint32_t four[2] = {0, 0};
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int t = t0 + 2 * tp + h;
            if (t < T && o < Mw) {
                const int4 src = *reinterpret_cast<const int4*>(perm + 4 * (size_t)t);
                const uint8_t* row = codes + (size_t)o * K;
                four[h] = pk::codes_four(row[src.x], row[src.y], row[src.z], row[src.w]);
            }
        }
#pragma unroll
        for (int p = 0; p < BITS; ++p) lds[lds_row(p, ol) * PACK_STRIDE + tp] = (uint8_t)(pk::codes_nibble(four[0], p) | (pk::codes_nibble(four[1], p) << 4));
    }
    __syncthreads();
    pack_store_tile<BITS>(lds, A_out, Mw, T, bm, kfactor);
}

// ---- BitNet master weights: W [Mw][K] in fp32, fp16 or bf16 -> levels -> the 2-bit blob (the absmean rule: tmac_pack.h) -------------------
// four masters of consecutive k (e: element index, a multiple of 4) as fp32, exactly: one 16-byte load of fp32, one 8-byte load of fp16 / bf16
template <int SRC>
__device__ __forceinline__ void load_masters(const void* __restrict__ W, size_t e, float (&w)[4]) {
    if constexpr (SRC == pk::SRC_F32) {
        const float4 v = *reinterpret_cast<const float4*>(static_cast<const float*>(W) + e);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    } else {
        const uint2 v = *reinterpret_cast<const uint2*>(static_cast<const uint16_t*>(W) + e);
        const uint16_t h[4] = {(uint16_t)v.x, (uint16_t)(v.x >> 16), (uint16_t)v.y, (uint16_t)(v.y >> 16)};
#pragma unroll
        for (int i = 0; i < 4; ++i) w[i] = SRC == pk::SRC_F16 ? __half2float(__ushort_as_half(h[i])) : pk::bf16_bits_to_f32(h[i]);
    }
}

// The scale, stage A: workgroup (row block g, chunk c) sums |w| over elements [c ABSMEAN_CHUNK, (c + 1) ABSMEAN_CHUNK) of the block -- a
// row block is block_elems = (Mw / m_groups) K consecutive elements, a multiple of 4 -- in fp64 into partials[g chunks + c].  A lane adds
// its ABSMEAN_STEPS loads in order, the 64 lanes of a wave meet in a xor butterfly (both partners form the same sum: addition commutes),
// the waves are added in index order.  No atomics: the bits depend on (block_elems, the data) alone.
template <int SRC>
__global__ __launch_bounds__(pk::ABSMEAN_THREADS) void k_absmean(const void* __restrict__ W, double* __restrict__ partials, size_t block_elems, unsigned chunks) {
    __shared__ double wave_sum[pk::ABSMEAN_THREADS / 64];
    const unsigned g = blockIdx.x / chunks, c = blockIdx.x % chunks;
    const size_t base = (size_t)g * block_elems, c0 = (size_t)c * pk::ABSMEAN_CHUNK;
    double acc = 0.0;
#pragma unroll 4
    for (int i = 0; i < pk::ABSMEAN_STEPS; ++i) {
        const size_t e = c0 + ((size_t)i * pk::ABSMEAN_THREADS + threadIdx.x) * pk::ABSMEAN_VEC;
        if (e < block_elems) {
            float w[4];
            load_masters<SRC>(W, base + e, w);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc += (double)fabsf(w[j]);
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off);
    if (threadIdx.x % 64 == 0) wave_sum[threadIdx.x / 64] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double sum = wave_sum[0];
#pragma unroll
        for (int v = 1; v < pk::ABSMEAN_THREADS / 64; ++v) sum += wave_sum[v];
        partials[blockIdx.x] = sum;
    }
}

// stage B: one workgroup per row block adds the block's chunk sums in index order (256 at a time through LDS, added by thread 0) and
// writes s = fmaxf(fp32(sum / count), eps)
__global__ __launch_bounds__(256) void k_absmean_scales(const double* __restrict__ partials, unsigned chunks, double count, float eps, float* __restrict__ scales_out) {
    __shared__ double tile[256];
    const double* p = partials + (size_t)blockIdx.x * chunks;
    double sum = 0.0;
    for (unsigned c0 = 0; c0 < chunks; c0 += 256) {
        const unsigned n = chunks - c0 < 256u ? chunks - c0 : 256u;
        if (threadIdx.x < n) tile[threadIdx.x] = p[c0 + threadIdx.x];
        __syncthreads();
        if (threadIdx.x == 0)
            for (unsigned i = 0; i < n; ++i) sum += tile[i];
        __syncthreads();
    }
    if (threadIdx.x == 0) scales_out[blockIdx.x] = pk::absmean_scale(sum, count, eps);
}

// k_pack_codes_weights<2> with another stage 1: the lane that took the four code bytes of a table takes its four masters and quantises
// them (pk::absmean_four) into the same `four`; no [Mw][K] code tensor exists anywhere.  scales: fp32 [Mw / rows_per_scale], the s of each
// row block.  A wave's step is one weight row, so the row block's scale is one scalar load per weight row.
template <int SRC>
__global__ __launch_bounds__(PACK_THREADS) void k_pack_dense_weights(const void* __restrict__ W, const float* __restrict__ scales, int rows_per_scale,
                                                                     uint8_t* __restrict__ A_out, int Mw, int K, int bm, int kfactor) {
    constexpr int BITS = 2;
    __shared__ __attribute__((aligned(16))) uint8_t lds[PACK_ROWS * BITS * PACK_STRIDE];
    const int T = K / 4;
    const int o0 = blockIdx.y * PACK_ROWS, t0 = blockIdx.x * PACK_TABLES;
    for (int idx = threadIdx.x; idx < PACK_ROWS * PACK_TABLES; idx += PACK_THREADS) {
        const int ol = idx / PACK_TABLES, tl = idx % PACK_TABLES;
        const int o = o0 + ol, t = t0 + tl;
        uint32_t four = 0;
        if (o < Mw && t < T) {
            const float inv = pk::absmean_inv(scales[__builtin_amdgcn_readfirstlane(o / rows_per_scale)]);     // o is the wave's
            float w[4];
            load_masters<SRC>(W, (size_t)o * K + 4 * (size_t)t, w);      // K is a multiple of 4
            four = pk::absmean_four(w[0], w[1], w[2], w[3], inv);
        }
#pragma unroll
        for (int p = 0; p < BITS; ++p) {
            uint32_t v = pk::codes_nibble(four, p) << (4 * (tl % 8));
            v |= __shfl_xor(v, 1);
            v |= __shfl_xor(v, 2);
            v |= __shfl_xor(v, 4);
            if (tl % 8 == 0) *reinterpret_cast<uint32_t*>(lds + lds_row(p, ol) * PACK_STRIDE + tl / 2) = v;
        }
    }
    __syncthreads();
    pack_store_tile<BITS>(lds, A_out, Mw, T, bm, kfactor);
}

// ---- BitNet packed ternary checkpoints: packed uint8 [R4][K], four weight rows per byte (the format: tmac_pack.h) ------------------------
// Fields of value 3, which have no level: a lane counts its own (`bad`), a wave adds its lanes' counts with shuffles and leaves the sum in
// `wave_bad` IN FRONT of the kernel's barrier between the stages; behind it thread 0 adds the waves' sums and, when the workgroup saw any,
// adds them to *counter with one atomicAdd.  counter == NULL: nothing is counted (uniform over the launch).
__device__ __forceinline__ void invalid_fold(int bad, int* wave_bad, const int32_t* counter) {
    if (!counter) return;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) bad += __shfl_xor(bad, off);
    if (threadIdx.x % 64 == 0) wave_bad[threadIdx.x / 64] = bad;
}
__device__ __forceinline__ void invalid_report(const int* wave_bad, int32_t* counter) {
    if (!counter || threadIdx.x != 0) return;
    int sum = 0;
#pragma unroll
    for (int v = 0; v < PACK_THREADS / 64; ++v) sum += wave_bad[v];
    if (sum) atomicAdd(counter, sum);
}

// The general form: k_pack_codes_weights<2> with another stage 1 -- the lane that took the four code bytes of (weight row o, table t) takes
// the four packed bytes of (packed row o % R4, table t) and extracts field o / R4.  Every Mw registration accepts (a multiple of 16, so R4
// is whole); each source byte is read from four tiles.  No [Mw][K] code tensor exists anywhere.
__global__ __launch_bounds__(PACK_THREADS) void k_pack_ternary_weights(const uint8_t* __restrict__ packed, uint8_t* __restrict__ A_out, int32_t* __restrict__ invalid,
                                                                       int Mw, int K, int bm, int kfactor) {
    constexpr int BITS = 2;
    __shared__ __attribute__((aligned(16))) uint8_t lds[PACK_ROWS * BITS * PACK_STRIDE];
    __shared__ int wave_bad[PACK_THREADS / 64];
    const int T = K / 4, R4 = Mw / 4;
    const int o0 = blockIdx.y * PACK_ROWS, t0 = blockIdx.x * PACK_TABLES;
    int bad = 0;
    for (int idx = threadIdx.x; idx < PACK_ROWS * PACK_TABLES; idx += PACK_THREADS) {
        const int ol = idx / PACK_TABLES, tl = idx % PACK_TABLES;
        const int o = o0 + ol, t = t0 + tl;
        uint32_t four = 0;
        if (o < Mw && t < T) {
            const uint32_t bytes = *reinterpret_cast<const uint32_t*>(packed + (size_t)pk::ternary_packed_row(o, R4) * K + 4 * (size_t)t);   // K is a multiple of 4
            int n;
            four = pk::ternary_four(bytes, pk::ternary_field(o, R4), &n);
            bad += n;
        }
#pragma unroll
        for (int p = 0; p < BITS; ++p) {
            uint32_t v = pk::codes_nibble(four, p) << (4 * (tl % 8));
            v |= __shfl_xor(v, 1);
            v |= __shfl_xor(v, 2);
            v |= __shfl_xor(v, 4);
            if (tl % 8 == 0) *reinterpret_cast<uint32_t*>(lds + lds_row(p, ol) * PACK_STRIDE + tl / 2) = v;
        }
    }
    invalid_fold(bad, wave_bad, invalid);
    __syncthreads();
    invalid_report(wave_bad, invalid);
    pack_store_tile<BITS>(lds, A_out, Mw, T, bm, kfactor);
}

// The read-once form, for R4 a multiple of 16: no group of 32 M-space rows (16 weight rows) then straddles two fields.  One workgroup loads
// a tile of 64 packed rows x 64 tables ONCE, 16 bytes (four tables) per lane along k -- K is a multiple of 32 (make_shape: K / 4 of
// kfactor, K of the activation group), so every such load is aligned and lies inside its row -- splits every byte into its four fields,
// fills four LDS tiles (one per field: 4 x 2 planes x 64 rows x PACK_STRIDE bytes) and runs stage 2 four times, once per output tile at
// weight rows i R4 + pr0 ...  The two lanes that hold the eight tables of an LDS word OR their halves together (one xor shuffle), one
// 32-bit store per (field, plane); every lane runs every step.  Tails: packed rows >= R4 and tables >= T load nothing and store nothing.
__global__ __launch_bounds__(PACK_THREADS) void k_pack_ternary_weights_x4(const uint8_t* __restrict__ packed, uint8_t* __restrict__ A_out,
                                                                          int32_t* __restrict__ invalid, int Mw, int K, int bm, int kfactor) {
    constexpr int BITS = 2, TILE = PACK_ROWS * BITS * PACK_STRIDE, LANES = PACK_TABLES / 4;      // LANES: 16-byte loads per packed row of the tile
    __shared__ __attribute__((aligned(16))) uint8_t lds[4 * TILE];
    __shared__ int wave_bad[PACK_THREADS / 64];
    const int T = K / 4, R4 = Mw / 4;
    const int pr0 = blockIdx.y * PACK_ROWS, t0 = blockIdx.x * PACK_TABLES;
    int bad = 0;
    for (int idx = threadIdx.x; idx < PACK_ROWS * LANES; idx += PACK_THREADS) {
        const int prl = idx / LANES, q = idx % LANES;
        const int pr = pr0 + prl, t = t0 + 4 * q;
        uint4 w4 = make_uint4(0, 0, 0, 0);
        if (pr < R4 && t < T) w4 = *reinterpret_cast<const uint4*>(packed + (size_t)pr * K + 4 * (size_t)t);      // T is a multiple of 8: whole quads of tables
        const uint32_t w[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            uint32_t nib[BITS] = {};          // the nibbles of the lane's four tables, lowest table first
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                int n;
                const uint32_t four = pk::ternary_four(w[j], i, &n);
                bad += n;
#pragma unroll
                for (int p = 0; p < BITS; ++p) nib[p] |= pk::codes_nibble(four, p) << (4 * j);
            }
#pragma unroll
            for (int p = 0; p < BITS; ++p) {
                uint32_t v = nib[p] << (16 * (q % 2));
                v |= __shfl_xor(v, 1);
                if (q % 2 == 0) *reinterpret_cast<uint32_t*>(lds + i * TILE + lds_row(p, prl) * PACK_STRIDE + 2 * q) = v;
            }
        }
    }
    invalid_fold(bad, wave_bad, invalid);
    __syncthreads();
    invalid_report(wave_bad, invalid);
    // output tile i: weight rows i R4 + pr0 ..., i.e. groups of 16 weight rows from (i R4 + pr0) / 16; field i ends at group (i + 1) R4 / 16
#pragma unroll
    for (int i = 0; i < 4; ++i) pack_store_groups<BITS>(lds + i * TILE, A_out, (i * R4 + pr0) / 16, (i + 1) * (R4 / 16), T, bm, kfactor);
}

// ---- AutoAWQ: qweight int32 [K][Mw / 8], eight weight rows per word along the OUTPUT axis, interleaved (the format: tmac_pack.h) ----------
// A word holds one column of eight weight rows, and a byte of the LDS image is eight consecutive columns of ONE row and plane.  A thread
// owns (V octets of weight rows, a pair of tables) and loads its 8 x V words (V = 4: one 16-byte load per k, for Mw a multiple of 32,
// where every qweight row is 16-byte aligned; V = 1: word loads, any Mw a multiple of 8).  Per octet and plane it folds the four words of
// each table into eight nibbles in field order (pk::awq_plane_nibbles: four shift-and-mask steps), takes row j's nibble of both tables
// from field INV[j] (pk::awq_plane_byte) and writes the 32 x V bytes of (plane, row of the octets, its table pair) itself: one writer per
// LDS byte, no shuffles.  Consecutive
// threads take consecutive octets of one table pair, so a load instruction of a wave runs along the words of a qweight row.
// TILES output tiles of 64 weight rows per workgroup, one LDS image each, stage 2 once per image (as k_pack_ternary_weights_x4):
// 8 TILES words = 32 TILES contiguous bytes of every qweight row of the tile.  Tails: octets >= Mw / 8 and columns >= K load nothing
// (a column >= K counts as zeros, in a byte whose upper table stage 2 does not store); stage 2 stores nothing past Mw / 8 groups or T tables.
constexpr int AWQ_TILES = 4;               // 64-row output tiles per workgroup: 32 octets = one 128-byte line of every qweight row
template <int V>
__global__ __launch_bounds__(PACK_THREADS) void k_pack_awq_weights(const uint32_t* __restrict__ qweight, uint8_t* __restrict__ A_out, int Mw, int K,
                                                                   int bm, int kfactor) {
    constexpr int BITS = 4, TILES = AWQ_TILES, TILE = PACK_ROWS * BITS * PACK_STRIDE, OCTETS = TILES * PACK_ROWS / 8, LOADS = OCTETS / V;
    static_assert(V == 1 || V == 4, "word loads or 16-byte loads");
    __shared__ __attribute__((aligned(16))) uint8_t lds[TILES * TILE];
    const int T = K / 4, MO = Mw / 8;      // MO: octets of weight rows = words per qweight row = groups of 32 M-space rows
    const int c0 = blockIdx.y * OCTETS, k0 = blockIdx.x * (PACK_TABLES * 4);
    for (int idx = threadIdx.x; idx < LOADS * (PACK_TABLES / 2); idx += PACK_THREADS) {
        const int tp = idx / LOADS, cl = (idx % LOADS) * V;
        const int c = c0 + cl;
        if (c >= MO) continue;              // V = 4: MO is a multiple of 4, so are c0 and cl -- a quad is inside the row or outside it
        uint32_t w[V][8];
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) {
            const int k = k0 + 8 * tp + kk;
            if constexpr (V == 4) {
                uint4 w4 = make_uint4(0, 0, 0, 0);
                if (k < K) w4 = *reinterpret_cast<const uint4*>(qweight + (size_t)k * MO + c);
                w[0][kk] = w4.x; w[1][kk] = w4.y; w[2][kk] = w4.z; w[3][kk] = w4.w;
            } else {
                w[0][kk] = k < K ? qweight[(size_t)k * MO + c] : 0u;
            }
        }
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const int row0 = (cl + v) * 8;          // the octet's first weight row, counted from the workgroup's
            uint8_t* img = lds + (row0 / PACK_ROWS) * TILE;
#pragma unroll
            for (int p = 0; p < BITS; ++p) {
                const uint32_t lo = pk::awq_plane_nibbles(w[v][0], w[v][1], w[v][2], w[v][3], p), hi = pk::awq_plane_nibbles(w[v][4], w[v][5], w[v][6], w[v][7], p);
#pragma unroll
                for (int j = 0; j < 8; ++j) img[lds_row(p, row0 % PACK_ROWS + j) * PACK_STRIDE + tp] = (uint8_t)pk::awq_plane_byte(lo, hi, j);
            }
        }
    }
    __syncthreads();
    // output tile i: weight rows 8 c0 + 64 i ..., i.e. groups from c0 + 8 i; the matrix ends at group MO
#pragma unroll
    for (int i = 0; i < TILES; ++i) pack_store_groups<BITS>(lds + i * TILE, A_out, c0 + i * (PACK_ROWS / 8), MO, T, bm, kfactor);
}

// ---- dense master weights -> W1 - W4 with per-group scales: round to nearest (the rule: tmac_pack.h) -------------------------------------
// EPL masters of consecutive k as fp32, exactly, in one 16-byte load: 4 of fp32, 8 of fp16 / bf16.  EPL = 4 of a 16-bit dtype (group sizes
// that are no multiple of 8): load_masters' 8-byte load.
template <int SRC, int EPL>
__device__ __forceinline__ void load_masters_vec(const void* __restrict__ W, size_t e, float (&w)[EPL]) {
    if constexpr (EPL == 4) {
        load_masters<SRC>(W, e, w);
    } else {
        static_assert(SRC != pk::SRC_F32 && EPL == 8, "16 bytes per load");
        const uint4 v = *reinterpret_cast<const uint4*>(static_cast<const uint16_t*>(W) + e);
        const uint32_t u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const uint16_t h = (uint16_t)(u[i / 2] >> (16 * (i % 2)));
            w[i] = SRC == pk::SRC_F16 ? __half2float(__ushort_as_half(h)) : pk::bf16_bits_to_f32(h);
        }
    }
}

// The parameters: item = (weight row o, group sg) = o SG + sg owns the gs CONSECUTIVE masters [item gs, (item + 1) gs) of the row-major
// matrix, and element `item` of each output (pk::rtn_param_index).  seg lanes (a power of two, <= 64: the host picks the smallest that
// covers gs / EPL loads, or 64) share an item and a wave takes 64 / seg consecutive items per step: where seg EPL == gs -- gs 64 to 256
// of fp32, 128 to 512 of fp16 / bf16 -- a step is one contiguous run of 64 16-byte loads.  min, max and "every master finite" meet in a
// xor butterfly over the item's lanes; minimum and maximum are exact, so no order shows.  The loop bound is the wave's: every lane runs
// every step.  Grid-stride over the items; nothing is read or written beyond `items`.  zeros (T-MAC's, for k_pack_codes_scales) may be
// NULL; invalid groups are counted as the ternary pack counts (invalid_fold / invalid_report).
template <int SRC, int EPL>
__global__ __launch_bounds__(PACK_THREADS) void k_rtn_params(const void* __restrict__ W, float* __restrict__ scales, float* __restrict__ zq,
                                                             float* __restrict__ zeros, int32_t* __restrict__ invalid, size_t items, int gs, int seg,
                                                             int bits, int zero_point, int scale_f16) {
    __shared__ int wave_bad[PACK_THREADS / 64];
    const int lane = threadIdx.x % 64, sub = lane % seg, gl = lane / seg, per_wave = 64 / seg, vecs = gs / EPL;
    const size_t wave = (size_t)blockIdx.x * (PACK_THREADS / 64) + threadIdx.x / 64, stride = (size_t)gridDim.x * (PACK_THREADS / 64) * per_wave;
    int bad = 0;
    for (size_t first = wave * per_wave; first < items; first += stride) {
        const size_t item = first + gl;
        float lo = 0.0f, hi = 0.0f, nf = 0.0f;      // nf: 0 while every master is finite (w * 0 is NaN for an infinity and for a NaN)
        if (item < items)
            for (int v = sub; v < vecs; v += seg) {
                float w[EPL];
                load_masters_vec<SRC, EPL>(W, item * gs + (size_t)v * EPL, w);
#pragma unroll
                for (int j = 0; j < EPL; ++j) {
                    lo = fminf(lo, w[j]);
                    hi = fmaxf(hi, w[j]);
                    nf = __fmaf_rn(w[j], 0.0f, nf);
                }
            }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1)
            if (off < seg) {
                lo = fminf(lo, __shfl_xor(lo, off));
                hi = fmaxf(hi, __shfl_xor(hi, off));
                nf += __shfl_xor(nf, off);
            }
        if (sub == 0 && item < items) {
            float s, z;
            if (!pk::rtn_scale_zq(lo, hi, nf == 0.0f, bits, zero_point, scale_f16, &s, &z)) ++bad;
            scales[item] = s;
            zq[item] = z;
            if (zeros) zeros[item] = pk::rtn_zero(s, z, bits);
        }
    }
    invalid_fold(bad, wave_bad, invalid);
    __syncthreads();
    invalid_report(wave_bad, invalid);
}

// k_pack_codes_weights<BITS> with another stage 1: the lane that took the four code bytes of a table takes its four masters and quantises
// them (pk::rtn_four) with the (scale, zq) of its row and group -- gs is a multiple of 4, so a table lies in one group; the lanes of a
// group load the same two words.  No [Mw][K] code tensor exists anywhere.
template <int SRC, int BITS>
__global__ __launch_bounds__(PACK_THREADS) void k_pack_rtn_weights(const void* __restrict__ W, const float* __restrict__ scales, const float* __restrict__ zq,
                                                                   uint8_t* __restrict__ A_out, int Mw, int K, int gs, int bm, int kfactor) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[PACK_ROWS * BITS * PACK_STRIDE];
    const int T = K / 4, SG = K / gs;
    const int o0 = blockIdx.y * PACK_ROWS, t0 = blockIdx.x * PACK_TABLES;
    for (int idx = threadIdx.x; idx < PACK_ROWS * PACK_TABLES; idx += PACK_THREADS) {
        const int ol = idx / PACK_TABLES, tl = idx % PACK_TABLES;
        const int o = o0 + ol, t = t0 + tl;
        uint32_t four = 0;
        if (o < Mw && t < T) {
            const size_t pi = pk::rtn_param_index(o, 4 * t / gs, SG);
            float w[4];
            load_masters<SRC>(W, (size_t)o * K + 4 * (size_t)t, w);      // K is a multiple of 4
            four = pk::rtn_four(w[0], w[1], w[2], w[3], scales[pi], zq[pi], BITS);
        }
#pragma unroll
        for (int p = 0; p < BITS; ++p) {
            uint32_t v = pk::codes_nibble(four, p) << (4 * (tl % 8));
            v |= __shfl_xor(v, 1);
            v |= __shfl_xor(v, 2);
            v |= __shfl_xor(v, 4);
            if (tl % 8 == 0) *reinterpret_cast<uint32_t*>(lds + lds_row(p, ol) * PACK_STRIDE + tl / 2) = v;
        }
    }
    __syncthreads();
    pack_store_tile<BITS>(lds, A_out, Mw, T, bm, kfactor);
}

// ---- scales -------------------------------------------------------------------------------------------------------------------------
// n contiguous elements (a multiple of 16 bytes, 16-byte aligned on both sides) as 16-byte accesses
template <class T, int N>
__device__ __forceinline__ void load_vec(const T* src, T (&v)[N]) {
    static_assert(sizeof(T) * N % 16 == 0, "whole 16-byte accesses");
    uint4 raw[sizeof(T) * N / 16];
#pragma unroll
    for (int i = 0; i < (int)(sizeof(T) * N / 16); ++i) raw[i] = reinterpret_cast<const uint4*>(src)[i];
    __builtin_memcpy(v, raw, sizeof(raw));
}
template <class T, int N>
__device__ __forceinline__ void store_vec(T* dst, const T (&v)[N]) {
    static_assert(sizeof(T) * N % 16 == 0, "whole 16-byte accesses");
    uint4 raw[sizeof(T) * N / 16];
    __builtin_memcpy(raw, v, sizeof(raw));
#pragma unroll
    for (int i = 0; i < (int)(sizeof(T) * N / 16); ++i) reinterpret_cast<uint4*>(dst)[i] = raw[i];
}

// the octet's 8 scales (and 8 zeros) -> scales_ref
template <class OT>
__device__ __forceinline__ void store_octet(OT* out, int o, int sg, const float (&sc)[8], const float (&zr)[8], int bm, int bits, int SG, int zero_point) {
    OT v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = from_f32<OT>(sc[i]);
    store_vec(out + pk::scale_index(o, sg, 0, bm, bits, SG, zero_point), v);
    if (zero_point) {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = from_f32<OT>(zr[i]);
        store_vec(out + pk::scale_index(o, sg, 1, bm, bits, SG, zero_point), v);
    }
}

// GPTQ: scales ST [SG][Mw], qzeros int32 [SG][Mw * bits / 32] (NULL without zero points); consecutive threads take consecutive octets
template <class ST, class OT>
__global__ __launch_bounds__(256) void k_pack_gptq_scales(const ST* __restrict__ scales, const uint32_t* __restrict__ qzeros, int v1, OT* __restrict__ out,
                                                         int Mw, int SG, int bits, int bm) {
    const int noct = Mw / 8;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)SG * noct) return;
    const int sg = (int)(idx / noct), o = (int)(idx % noct) * 8;
    ST s[8];
    load_vec(scales + (size_t)sg * Mw + o, s);
    float sc[8], zr[8];
    uint32_t zw = 0;
    if (qzeros) zw = qzeros[(size_t)sg * (Mw * bits / 32) + o * bits / 32] >> (o * bits % 32);   // 8 fields of an octet never straddle a word
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        sc[i] = to_f32(s[i]);
        // one rounding to the scales' dtype (tmac_pack.h): fp32 scales -- the fp32 product; fp16 scales -- the exact product, rounded once
        zr[i] = to_f32(from_f32<ST>(pk::gptq_zero_multiplier(pk::gptq_field(zw, i, bits), v1, bits) * sc[i]));
    }
    store_octet(out, o, sg, sc, zr, bm, bits, SG, qzeros != nullptr);
}

// AutoAWQ: k_pack_gptq_scales at 4 bits with the zero of row o + i taken from field INV[i] of the octet's word -- scales ST [SG][Mw],
// qzeros int32 [SG][Mw / 8] (NULL without zero points), the stored zero is z itself
template <class ST, class OT>
__global__ __launch_bounds__(256) void k_pack_awq_scales(const ST* __restrict__ scales, const uint32_t* __restrict__ qzeros, OT* __restrict__ out, int Mw,
                                                        int SG, int bm) {
    constexpr int BITS = 4;
    const int noct = Mw / 8;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)SG * noct) return;
    const int sg = (int)(idx / noct), o = (int)(idx % noct) * 8;
    ST s[8];
    load_vec(scales + (size_t)sg * Mw + o, s);
    float sc[8], zr[8];
    const uint32_t zw = qzeros ? qzeros[idx] : 0u;      // word (sg, o / 8)
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        sc[i] = to_f32(s[i]);
        zr[i] = to_f32(from_f32<ST>(pk::gptq_zero_multiplier(pk::awq_code(zw, i), 0, BITS) * sc[i]));     // one rounding, to the scales' dtype
    }
    store_octet(out, o, sg, sc, zr, bm, BITS, SG, qzeros != nullptr);
}

// codes form: scales / zeros ST [Mw][SG], already in T-MAC's convention; consecutive threads take consecutive scale groups
template <class ST, class OT>
__global__ __launch_bounds__(256) void k_pack_codes_scales(const ST* __restrict__ scales, const ST* __restrict__ zeros, OT* __restrict__ out, int Mw, int SG,
                                                          int bits, int bm) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)SG * (Mw / 8)) return;
    const int sg = (int)(idx % SG), o = (int)(idx / SG) * 8;
    float sc[8], zr[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        sc[i] = to_f32(scales[(size_t)(o + i) * SG + sg]);
        zr[i] = zeros ? to_f32(zeros[(size_t)(o + i) * SG + sg]) : 0.0f;
    }
    store_octet(out, o, sg, sc, zr, bm, bits, SG, zeros != nullptr);
}

template <class ST, class OT>
__global__ void k_pack_copy(const ST* __restrict__ in, OT* __restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = from_f32<OT>(to_f32(in[i]));
}

// instantiates `launch`, a generic lambda taking two value-less type tags, for the (input, output) dtype pair
template <class F>
void by_dtypes(Dtype in_dt, Dtype out_dt, F&& launch) {
    if (in_dt == F32 && out_dt == F32) launch(float(), float());
    else if (in_dt == F32) launch(float(), __half());
    else if (out_dt == F32) launch(__half(), float());
    else launch(__half(), __half());
}

dim3 weight_grid(const Shape& s) { return dim3((unsigned)((s.K / 4 + PACK_TABLES - 1) / PACK_TABLES), (unsigned)((s.Mw + PACK_ROWS - 1) / PACK_ROWS)); }

}  // namespace

hipError_t launch_pack_gptq(const void* qweight, const void* scales, const void* qzeros, Dtype scales_dt, int gptq_v2, void* A_out, void* S_out,
                            Dtype out_dt, const Shape& s, hipStream_t st, const int32_t* perm) {
    const dim3 g = weight_grid(s), b(PACK_THREADS);
    const uint32_t* qw = (const uint32_t*)qweight;
    uint8_t* A = (uint8_t*)A_out;
    if (!perm) switch (s.bits) {
        case 1: hipLaunchKernelGGL(k_pack_gptq_weights<1>, g, b, 0, st, qw, A, s.Mw, s.K, s.bm, s.kfactor); break;
        case 2: hipLaunchKernelGGL(k_pack_gptq_weights<2>, g, b, 0, st, qw, A, s.Mw, s.K, s.bm, s.kfactor); break;
        case 4: hipLaunchKernelGGL(k_pack_gptq_weights<4>, g, b, 0, st, qw, A, s.Mw, s.K, s.bm, s.kfactor); break;
        default: return hipErrorInvalidValue;
    }
    else switch (s.bits) {      // act-order: stage 1 through the permutation
        case 1: hipLaunchKernelGGL(k_pack_gptq_weights_perm<1>, g, b, 0, st, qw, perm, A, s.Mw, s.K, s.bm, s.kfactor); break;
        case 2: hipLaunchKernelGGL(k_pack_gptq_weights_perm<2>, g, b, 0, st, qw, perm, A, s.Mw, s.K, s.bm, s.kfactor); break;
        case 4: hipLaunchKernelGGL(k_pack_gptq_weights_perm<4>, g, b, 0, st, qw, perm, A, s.Mw, s.K, s.bm, s.kfactor); break;
        default: return hipErrorInvalidValue;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int SG = s.K / s.gs;
    const size_t n = (size_t)SG * (s.Mw / 8);
    by_dtypes(scales_dt, out_dt, [&](auto in_tag, auto out_tag) {
        using ST = decltype(in_tag);
        using OT = decltype(out_tag);
        hipLaunchKernelGGL((k_pack_gptq_scales<ST, OT>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const ST*)scales, (const uint32_t*)qzeros,
                           gptq_v2 ? 0 : 1, (OT*)S_out, s.Mw, SG, s.bits, s.bm);
    });
    return hipGetLastError();
}

// ---- AutoAWQ ---------------------------------------------------------------------------------------------------------------------------

hipError_t launch_pack_awq(const void* qweight, const void* scales, const void* qzeros, Dtype scales_dt, void* A_out, void* S_out, Dtype out_dt,
                           const Shape& s, hipStream_t st) {
    if (s.bits != 4 || s.m_groups >= 1 || s.Mw % 8) return hipErrorInvalidValue;
    const dim3 g((unsigned)((s.K / 4 + PACK_TABLES - 1) / PACK_TABLES), (unsigned)((s.Mw + AWQ_TILES * PACK_ROWS - 1) / (AWQ_TILES * PACK_ROWS))), b(PACK_THREADS);
    const uint32_t* qw = (const uint32_t*)qweight;
    uint8_t* A = (uint8_t*)A_out;
    // 16-byte loads where every qweight row is 16-byte aligned (Mw / 8 words, a multiple of 4), word loads otherwise
    if (s.Mw % 32 == 0) hipLaunchKernelGGL(k_pack_awq_weights<4>, g, b, 0, st, qw, A, s.Mw, s.K, s.bm, s.kfactor);
    else hipLaunchKernelGGL(k_pack_awq_weights<1>, g, b, 0, st, qw, A, s.Mw, s.K, s.bm, s.kfactor);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int SG = s.K / s.gs;
    const size_t n = (size_t)SG * (s.Mw / 8);
    by_dtypes(scales_dt, out_dt, [&](auto in_tag, auto out_tag) {
        using ST = decltype(in_tag);
        using OT = decltype(out_tag);
        hipLaunchKernelGGL((k_pack_awq_scales<ST, OT>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const ST*)scales, (const uint32_t*)qzeros,
                           (OT*)S_out, s.Mw, SG, s.bm);
    });
    return hipGetLastError();
}

hipError_t launch_pack_codes(const void* codes, const void* scales, const void* zeros, Dtype sz_dt, void* A_out, void* S_out, Dtype out_dt,
                             const Shape& s, hipStream_t st, const int32_t* perm) {
    const dim3 g = weight_grid(s), b(PACK_THREADS);
    const uint8_t* cd = (const uint8_t*)codes;
    uint8_t* A = (uint8_t*)A_out;
    if (!perm) switch (s.bits) {
        case 1: hipLaunchKernelGGL(k_pack_codes_weights<1>, g, b, 0, st, cd, A, s.Mw, s.K, s.bm, s.kfactor); break;
        case 2: hipLaunchKernelGGL(k_pack_codes_weights<2>, g, b, 0, st, cd, A, s.Mw, s.K, s.bm, s.kfactor); break;
        case 3: hipLaunchKernelGGL(k_pack_codes_weights<3>, g, b, 0, st, cd, A, s.Mw, s.K, s.bm, s.kfactor); break;
        case 4: hipLaunchKernelGGL(k_pack_codes_weights<4>, g, b, 0, st, cd, A, s.Mw, s.K, s.bm, s.kfactor); break;
        default: return hipErrorInvalidValue;
    }
    else switch (s.bits) {      // act-order: stage 1 through the permutation
        case 1: hipLaunchKernelGGL(k_pack_codes_weights_perm<1>, g, b, 0, st, cd, perm, A, s.Mw, s.K, s.bm, s.kfactor); break;
        case 2: hipLaunchKernelGGL(k_pack_codes_weights_perm<2>, g, b, 0, st, cd, perm, A, s.Mw, s.K, s.bm, s.kfactor); break;
        case 3: hipLaunchKernelGGL(k_pack_codes_weights_perm<3>, g, b, 0, st, cd, perm, A, s.Mw, s.K, s.bm, s.kfactor); break;
        case 4: hipLaunchKernelGGL(k_pack_codes_weights_perm<4>, g, b, 0, st, cd, perm, A, s.Mw, s.K, s.bm, s.kfactor); break;
        default: return hipErrorInvalidValue;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (s.m_groups >= 1) {      // unified scale(s): the m_groups values, copied
        const size_t n = (size_t)s.m_groups;
        by_dtypes(sz_dt, out_dt, [&](auto in_tag, auto out_tag) {
            using ST = decltype(in_tag);
            using OT = decltype(out_tag);
            hipLaunchKernelGGL((k_pack_copy<ST, OT>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const ST*)scales, (OT*)S_out, n);
        });
        return hipGetLastError();
    }
    const int SG = s.K / s.gs;
    const size_t n = (size_t)SG * (s.Mw / 8);
    by_dtypes(sz_dt, out_dt, [&](auto in_tag, auto out_tag) {
        using ST = decltype(in_tag);
        using OT = decltype(out_tag);
        hipLaunchKernelGGL((k_pack_codes_scales<ST, OT>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const ST*)scales, (const ST*)zeros, (OT*)S_out,
                           s.Mw, SG, s.bits, s.bm);
    });
    return hipGetLastError();
}

// ---- BitNet master weights ----------------------------------------------------------------------------------------------------------
size_t absmean_partial_count(int Mw, int K, int m_groups) { return pk::absmean_chunks((size_t)(Mw / m_groups) * K) * (size_t)m_groups; }

hipError_t launch_absmean(const void* W, int src, int Mw, int K, int m_groups, float eps, double* partials, float* scales_out, hipStream_t st) {
    const size_t block_elems = (size_t)(Mw / m_groups) * K, chunks = pk::absmean_chunks(block_elems), total = chunks * (size_t)m_groups;
    if (total > (size_t)INT32_MAX) return hipErrorInvalidValue;
    const dim3 g((unsigned)total), b(pk::ABSMEAN_THREADS);
    switch (src) {
        case pk::SRC_F32: hipLaunchKernelGGL(k_absmean<pk::SRC_F32>, g, b, 0, st, W, partials, block_elems, (unsigned)chunks); break;
        case pk::SRC_F16: hipLaunchKernelGGL(k_absmean<pk::SRC_F16>, g, b, 0, st, W, partials, block_elems, (unsigned)chunks); break;
        case pk::SRC_BF16: hipLaunchKernelGGL(k_absmean<pk::SRC_BF16>, g, b, 0, st, W, partials, block_elems, (unsigned)chunks); break;
        default: return hipErrorInvalidValue;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_absmean_scales, dim3((unsigned)m_groups), dim3(256), 0, st, (const double*)partials, (unsigned)chunks, (double)block_elems, eps,
                       scales_out);
    return hipGetLastError();
}

hipError_t launch_pack_dense(const void* W, int src, const float* scales, void* A_out, void* S_out, Dtype out_dt, const Shape& s, hipStream_t st) {
    if (s.bits != 2 || s.m_groups < 1) return hipErrorInvalidValue;
    const dim3 g = weight_grid(s), b(PACK_THREADS);
    const int R = s.Mw / s.m_groups;
    uint8_t* A = (uint8_t*)A_out;
    switch (src) {
        case pk::SRC_F32: hipLaunchKernelGGL(k_pack_dense_weights<pk::SRC_F32>, g, b, 0, st, W, scales, R, A, s.Mw, s.K, s.bm, s.kfactor); break;
        case pk::SRC_F16: hipLaunchKernelGGL(k_pack_dense_weights<pk::SRC_F16>, g, b, 0, st, W, scales, R, A, s.Mw, s.K, s.bm, s.kfactor); break;
        case pk::SRC_BF16: hipLaunchKernelGGL(k_pack_dense_weights<pk::SRC_BF16>, g, b, 0, st, W, scales, R, A, s.Mw, s.K, s.bm, s.kfactor); break;
        default: return hipErrorInvalidValue;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const size_t n = (size_t)s.m_groups;      // the unified scales into the blob: the copy of the codes form
    by_dtypes(F32, out_dt, [&](auto in_tag, auto out_tag) {
        using ST = decltype(in_tag);
        using OT = decltype(out_tag);
        hipLaunchKernelGGL((k_pack_copy<ST, OT>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const ST*)scales, (OT*)S_out, n);
    });
    return hipGetLastError();
}

// ---- dense master weights, round to nearest --------------------------------------------------------------------------------------------
hipError_t launch_rtn_params(const void* W, int src, int Mw, int K, int bits, int gs, int zero_point, int scale_f16, float* scales, float* zq, float* zeros,
                             int32_t* invalid, hipStream_t st) {
    if (bits < 1 || bits > 4 || gs <= 0 || gs % 4 || K % gs) return hipErrorInvalidValue;
    const size_t items = (size_t)Mw * (K / gs);
    const int epl = src != pk::SRC_F32 && gs % 8 == 0 ? 8 : 4, vecs = gs / epl;
    int seg = 1;
    while (seg < vecs && seg < 64) seg <<= 1;
    // memory bound: enough workgroups of four waves to cover the items once, at most 2048 of them (the rest by the grid stride)
    const size_t per_block = (size_t)(PACK_THREADS / 64) * (64 / seg), blocks = (items + per_block - 1) / per_block;
    const dim3 g((unsigned)(blocks < 2048 ? blocks : 2048)), b(PACK_THREADS);
    const int zp = zero_point ? 1 : 0, f16 = scale_f16 ? 1 : 0;
    if (src == pk::SRC_F32) hipLaunchKernelGGL((k_rtn_params<pk::SRC_F32, 4>), g, b, 0, st, W, scales, zq, zeros, invalid, items, gs, seg, bits, zp, f16);
    else if (src == pk::SRC_F16 && epl == 8) hipLaunchKernelGGL((k_rtn_params<pk::SRC_F16, 8>), g, b, 0, st, W, scales, zq, zeros, invalid, items, gs, seg, bits, zp, f16);
    else if (src == pk::SRC_F16) hipLaunchKernelGGL((k_rtn_params<pk::SRC_F16, 4>), g, b, 0, st, W, scales, zq, zeros, invalid, items, gs, seg, bits, zp, f16);
    else if (src == pk::SRC_BF16 && epl == 8) hipLaunchKernelGGL((k_rtn_params<pk::SRC_BF16, 8>), g, b, 0, st, W, scales, zq, zeros, invalid, items, gs, seg, bits, zp, f16);
    else if (src == pk::SRC_BF16) hipLaunchKernelGGL((k_rtn_params<pk::SRC_BF16, 4>), g, b, 0, st, W, scales, zq, zeros, invalid, items, gs, seg, bits, zp, f16);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

namespace {
template <int SRC>
hipError_t launch_pack_rtn_weights(const void* W, const float* scales, const float* zq, uint8_t* A, const Shape& s, hipStream_t st) {
    const dim3 g = weight_grid(s), b(PACK_THREADS);
    switch (s.bits) {
        case 1: hipLaunchKernelGGL((k_pack_rtn_weights<SRC, 1>), g, b, 0, st, W, scales, zq, A, s.Mw, s.K, s.gs, s.bm, s.kfactor); break;
        case 2: hipLaunchKernelGGL((k_pack_rtn_weights<SRC, 2>), g, b, 0, st, W, scales, zq, A, s.Mw, s.K, s.gs, s.bm, s.kfactor); break;
        case 3: hipLaunchKernelGGL((k_pack_rtn_weights<SRC, 3>), g, b, 0, st, W, scales, zq, A, s.Mw, s.K, s.gs, s.bm, s.kfactor); break;
        case 4: hipLaunchKernelGGL((k_pack_rtn_weights<SRC, 4>), g, b, 0, st, W, scales, zq, A, s.Mw, s.K, s.gs, s.bm, s.kfactor); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
}  // namespace

hipError_t launch_pack_rtn(const void* W, int src, const float* scales, const float* zq, const float* zeros, void* A_out, void* S_out, Dtype out_dt,
                           const Shape& s, hipStream_t st) {
    if (s.m_groups >= 1 || (zeros != nullptr) != (s.zero_point != 0)) return hipErrorInvalidValue;
    uint8_t* A = (uint8_t*)A_out;
    hipError_t e;
    switch (src) {
        case pk::SRC_F32: e = launch_pack_rtn_weights<pk::SRC_F32>(W, scales, zq, A, s, st); break;
        case pk::SRC_F16: e = launch_pack_rtn_weights<pk::SRC_F16>(W, scales, zq, A, s, st); break;
        case pk::SRC_BF16: e = launch_pack_rtn_weights<pk::SRC_BF16>(W, scales, zq, A, s, st); break;
        default: return hipErrorInvalidValue;
    }
    if (e != hipSuccess) return e;
    const int SG = s.K / s.gs;      // the parameters into the blob: the scales kernel of the codes form
    const size_t n = (size_t)SG * (s.Mw / 8);
    by_dtypes(F32, out_dt, [&](auto in_tag, auto out_tag) {
        using ST = decltype(in_tag);
        using OT = decltype(out_tag);
        hipLaunchKernelGGL((k_pack_codes_scales<ST, OT>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const ST*)scales, (const ST*)zeros, (OT*)S_out,
                           s.Mw, SG, s.bits, s.bm);
    });
    return hipGetLastError();
}

// ---- BitNet packed ternary checkpoints ------------------------------------------------------------------------------------------------
bool pack_ternary_reads_once(const Shape& s) { return (s.Mw / 4) % 16 == 0; }

hipError_t launch_pack_ternary(const void* packed, const float* scales, void* A_out, void* S_out, Dtype out_dt, const Shape& s, int32_t* invalid,
                               bool general, hipStream_t st) {
    if (s.bits != 2 || s.m_groups < 1) return hipErrorInvalidValue;
    const uint8_t* src = (const uint8_t*)packed;
    uint8_t* A = (uint8_t*)A_out;
    const dim3 b(PACK_THREADS);
    if (!general && pack_ternary_reads_once(s)) {
        const dim3 g((unsigned)((s.K / 4 + PACK_TABLES - 1) / PACK_TABLES), (unsigned)((s.Mw / 4 + PACK_ROWS - 1) / PACK_ROWS));
        hipLaunchKernelGGL(k_pack_ternary_weights_x4, g, b, 0, st, src, A, invalid, s.Mw, s.K, s.bm, s.kfactor);
    } else {
        hipLaunchKernelGGL(k_pack_ternary_weights, weight_grid(s), b, 0, st, src, A, invalid, s.Mw, s.K, s.bm, s.kfactor);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const size_t n = (size_t)s.m_groups;      // the unified scales into the blob: the copy of the codes form
    by_dtypes(F32, out_dt, [&](auto in_tag, auto out_tag) {
        using ST = decltype(in_tag);
        using OT = decltype(out_tag);
        hipLaunchKernelGGL((k_pack_copy<ST, OT>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const ST*)scales, (OT*)S_out, n);
    });
    return hipGetLastError();
}

// ---- a handle's bias (tmac_hip_weights_set_bias_dev) --------------------------------------------------------------------------------------
// bias [Mw] in fp32, fp16 or bf16 -> the handle's own fp32 copy out [Mpad]: the conversions are exact, elements Mw .. Mpad - 1 are zero (a
// 16-byte load at a tile's edge reads the library's zeros).  Element-wise loads: nothing outside [bias, bias + Mw) is read.
template <int SRC>
__global__ __launch_bounds__(256) void k_bias_copy(const void* __restrict__ bias, float* __restrict__ out, int Mw, int Mpad) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= Mpad) return;
    float v = 0.f;
    if (i < Mw) {
        if constexpr (SRC == pk::SRC_F32) v = static_cast<const float*>(bias)[i];
        else if constexpr (SRC == pk::SRC_F16) v = __half2float(__ushort_as_half(static_cast<const uint16_t*>(bias)[i]));
        else v = pk::bf16_bits_to_f32(static_cast<const uint16_t*>(bias)[i]);
    }
    out[i] = v;
}

hipError_t launch_bias_copy(const void* bias, int src, float* out, int Mw, int Mpad, hipStream_t st) {
    if (Mw < 1 || Mpad < Mw) return hipErrorInvalidValue;
    const dim3 g((unsigned)((Mpad + 255) / 256)), b(256);
    switch (src) {
        case pk::SRC_F32: hipLaunchKernelGGL(k_bias_copy<pk::SRC_F32>, g, b, 0, st, bias, out, Mw, Mpad); break;
        case pk::SRC_F16: hipLaunchKernelGGL(k_bias_copy<pk::SRC_F16>, g, b, 0, st, bias, out, Mw, Mpad); break;
        case pk::SRC_BF16: hipLaunchKernelGGL(k_bias_copy<pk::SRC_BF16>, g, b, 0, st, bias, out, Mw, Mpad); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace tmac
