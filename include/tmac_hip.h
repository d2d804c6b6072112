/*
 * tmac_hip.h — C-ABI of libtmac_hip.so: T-MAC's LUT mpGEMM hot path on MI355X (gfx950).
 *
 * Drop-in boundary.  Plain pointers and sizes only; every function returns
 * 0 on success, -1 when no kernel matches the requested shape/configuration (the reference's
 * dispatcher contract, deploy/tuned/<set>/kernels.h `return -1`), and < -1 for runtime
 * failures (tmac_hip_last_error() explains).  No CPU fallback exists: without a HIP device
 * every compute entry point fails with TMAC_HIP_E_NODEVICE.
 *
 * Three layers:
 *   (1) reference-named entry points taking HOST pointers in the reference's own layouts —
 *       what the llama.cpp fork binds today (generated kernels.h):
 *         preprocessor_int8 / qgemm_lut_int8 and the shape-named kernels.
 *   (2) device-resident extensions — weights registered (uploaded + re-tiled) once, LUT
 *       workspace on the GPU, launches on a caller-provided hipStream_t.  This is the path
 *       that is benchmarked; a per-call H2D copy of 11 MB would erase the point.
 *   (3) parity taps used by tests: read back QLUT / integer partial sums.
 *
 * float_type: the reference uses fp16 on ARM and fp32 on x86 (python/t_mac/intrins/tbl.cc:10-15).
 * Layer (1) follows the HOST's float_type (fp32 on the x86 hosts of MI355X boxes); layer (2)
 * takes an explicit dtype per tensor.
 */
#ifndef TMAC_HIP_H_
#define TMAC_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* libtmac_hip.so is built with -fvisibility=hidden: exactly what this header declares is exported */
#pragma GCC visibility push(default)

#define TMAC_HIP_OK 0
#define TMAC_HIP_E_NOMATCH (-1)   /* no kernel for this shape/config (reference: dispatcher returns -1) */
#define TMAC_HIP_E_NODEVICE (-2)  /* no usable HIP device */
#define TMAC_HIP_E_RUNTIME (-3)   /* a HIP call failed */
#define TMAC_HIP_E_ARG (-4)       /* invalid argument */

typedef enum { TMAC_F32 = 0, TMAC_F16 = 1 } tmac_dtype_t;

#define TMAC_HIP_ABI_VERSION 1   /* bumped when an exported signature changes */

/* Mirrors TMAC::TMACGeMMConfig (include/t-mac/tmac_gemm_wrapper.h:26-35) plus the three facts the
 * reference bakes into the compiled kernel instead of kcfg.ini (zero_point, act_group_size,
 * m_groups: python/t_mac/ops/qgemm.py:16-96). */
typedef struct tmac_kcfg {
    int bm;              /* M-tile in bit-plane rows                       (kcfg.ini: bm)        */
    int simd_n_in;       /* 16                                              (kcfg.ini)            */
    int simd_n_out;      /* 8                                               (kcfg.ini)            */
    int kfactor;         /* LUT groups per tbl call                         (kcfg.ini)            */
    int group_size;      /* weight quantisation group along K               (kcfg.ini)            */
    int lut_scales_size; /* N * K / act_group_size                          (kcfg.ini)            */
    int scales_size;     /* number of scale(+zero) values                   (kcfg.ini)            */
    int n_tile_num;      /* M / bm                                          (kcfg.ini)            */
    int act_group_size;  /* activations sharing one LUT scale (64; == K for BitNet on x86)       */
    int zero_point;      /* scales interleaved with zero points                                   */
    int m_groups;        /* -1: per-(row, group) scales; >=1: unified scale(s) (BitNet)           */
} tmac_kcfg;

typedef struct tmac_hip_weights tmac_hip_weights;      /* one registered weight matrix (device) */
typedef struct tmac_hip_workspace tmac_hip_workspace;  /* QLUT + LUT scales/biases (device)     */

/* ---- lifecycle ------------------------------------------------------------------------- */
int32_t tmac_hip_init(int device);            /* selects the device; idempotent               */
const char* tmac_hip_last_error(void);        /* thread-local message of the last failure     */
const char* tmac_hip_version(void);
int32_t tmac_hip_device_count(void);
/* 1 when p points into device memory (hipMalloc and friends), 0 for host memory of any kind (pageable, pinned) and for NULL.  For glue
 * code that receives tensors from a host framework and must decide between staging and passing the pointer on (src/ggml_tmac_hip.cc). */
int32_t tmac_hip_pointer_on_device(const void* p);

/* kcfg.ini handling: same file format and section names as the reference
 * (deploy/compile.py:153-165; lookup tmac_gemm_wrapper.h:230-255).  `path` NULL -> $TMAC_KCFG_FILE. */
int32_t tmac_hip_load_kcfg(const char* path);
/* replace != 0: the file becomes the whole table (the reference's runtime holds exactly one kcfg.ini); 0 merges as
 * tmac_hip_load_kcfg does.  tmac_hip_clear_kcfg empties the table.  The per-tile host-pointer entry points return -1 when
 * several loaded sections match their (bm, k, n, b) key and disagree on the quantisation layout. */
int32_t tmac_hip_load_kcfg_ex(const char* path, int replace);
int32_t tmac_hip_clear_kcfg(void);
/* Puts every piece of process-global state back to that of a freshly loaded library: kcfg table, tuning table, all
 * tmac_hip_set_* / tmac_hip_debug_* knobs, the host-pointer layer's caches, LUT workspace and staging buffers, the fused
 * entry point's per-stream workspaces, the calling thread's deferred mode (left, its queue launched first) and tmac_hip_defer_stats
 * counters.  Registered weights, workspaces and chains the caller holds stay valid.
 * Synchronises the library's own streams.  (tests/conftest.py calls it before every GPU test.) */
int32_t tmac_hip_reset_state(void);
/* M here is the number of WEIGHT rows (as in TMACGeMMWrapper::get_kcfg); fills zero_point /
 * act_group_size / m_groups from scales_size / lut_scales_size as the reference's shapes imply. */
int32_t tmac_hip_get_kcfg(int M, int K, int N, int bits, tmac_kcfg* out);
/* programmatic alternative to a file (used by tests and bench) */
int32_t tmac_hip_set_kcfg(int M, int K, int N, int bits, const tmac_kcfg* cfg);

/* ---- (2) device-resident path ---------------------------------------------------------- */

/* Alignment of the caller's DEVICE pointers.  The kernels read and write caller memory with vector accesses; a pointer below the widest
 * access it gets is refused with TMAC_HIP_E_ARG and a message naming the argument -- at once, also while recording a chain or with
 * deferral on (nothing is launched, recorded or queued; the queue and the recording stay as they were):
 *   B_dev (activations, fp16 or fp32; every entry point)       16 bytes  (every LUT build loads uint4 / float4; rows follow each other
 *                                                                         K elements apart, K is a multiple of 64: they stay aligned)
 *   C_dev, C_dev[i] (outputs)                 fp32: 16 bytes, fp16: 8    (the GEMMs store four outputs of a row at a time; Mw is a
 *                                                                         multiple of 4, so every row of [N][Mw] stays aligned)
 *   tmac_hip_xform: in2, residual, gamma, residual_out          16 bytes  (16-byte loads into LDS; residual_out: 16-byte stores)
 *   bias_dev (tmac_hip_weights_set_bias_dev)                    16 bytes  (copied once into the handle; the kernels read the copy)
 *   A_ref_dev, scales_ref_dev, the tap buffer of tmac_hip_chain_set_tap, recv / send of the exchange step: their element type
 *     (copied, or read and written element by element)
 * The rule goes by the argument's ROLE and dtype, not by the route a call takes: an fp32 C_dev needs 16 bytes for N = 1 too (where the
 * kernels of today store narrower; the dispatcher is free to pick another), and an output that a later call takes as its B_dev or in2
 * must satisfy THEIR 16 bytes as well -- also inside a recording, where the value travels through the hand-off image: the same pointers
 * must stay valid for launching the calls one by one.  An allocator that aligns every tensor to 16 bytes or more (hipMalloc: 256, ggml:
 * 32, torch: 512) never meets a refusal.
 * The tests hold the kernels to no more than this: a base that is 32-byte and not 64-byte aligned (ggml's tensor alignment) is served like a 256-byte one, bit for
 * bit (tests/test_gpu_footprint.py).  Host pointers (layer 1, the read-back taps) are copied and need the alignment of their element
 * type only.  Intended, and asserted by the same test file: no kernel writes anything outside [pointer, pointer + extent) of an output,
 * or lets a value from outside an input's extent reach a result. */

/* Upload + re-tile one weight matrix given in the REFERENCE layout (python/t_mac/weights.py:57-87):
 *   A_ref      uint8 [M/bm][K/4][bm/2]           (M = Mw*bits bit-plane rows)
 *   scales_ref float_type: zero_point [M/bm][K/gs][bm/bits/8][2][8]; else [M/bm][K/gs][bm/bits/8][8];
 *              m_groups>=1: [m_groups]
 * host_float : dtype of scales_ref (TMAC_F32 on x86 hosts, TMAC_F16 for ARM-produced blobs)
 * dev_float  : dtype the scales are STORED in on the GPU (TMAC_F16 halves their HBM traffic and is
 *              exact when the values are fp16-representable; TMAC_F32 keeps x86 bit parity)
 * The re-tiling is a pure permutation of nibbles (+ a bijective recoding of each nibble), so every
 * integer partial sum is identical to the reference's.  Row shards for multi-GPU: pass the tile
 * pointers of the shard and its Mw (tiles are contiguous in the reference layout). */
int32_t tmac_hip_register_weights(tmac_hip_weights** out, const void* A_ref, const void* scales_ref,
                                  int Mw, int K, int bits, const tmac_kcfg* cfg,
                                  tmac_dtype_t host_float, tmac_dtype_t dev_float, void* stream);
/* Same, but A_ref / scales_ref already live in device memory (bench: avoids a 1.6 GB PCIe upload). */
int32_t tmac_hip_register_weights_dev(tmac_hip_weights** out, const void* A_ref_dev, const void* scales_ref_dev,
                                      int Mw, int K, int bits, const tmac_kcfg* cfg,
                                      tmac_dtype_t host_float, tmac_dtype_t dev_float, void* stream);
int32_t tmac_hip_free_weights(tmac_hip_weights* w);
/* bytes one GEMV must read from HBM for this matrix (weights + scales), i.e. SURVEY.md §8d's
 * algorithmic bytes minus the activation-side terms */
size_t tmac_hip_weights_bytes(const tmac_hip_weights* w);

/* ---- device-side packing: checkpoint tensors -> reference blob -> handle, without the host -------------------------------
 * A quantised checkpoint holds no blob: it holds GPTQ tensors, or codes with scales.  The blob is a pure permutation of their bits
 * (python/t_mac/weights.py:57-87), so tensors that are in device memory are packed there (k_pack_* in tmac_pack.hip: every input word read
 * once, the [k][m] -> row-interleaved transposition through LDS, one writer per output byte) instead of by the host.  Two input forms:
 *   GPTQ    qweight int32 [K*bits/32][Mw]   row kp packs k = kp*(32/bits) ... of column m, lowest field first
 *           scales  scales_dtype [K/gs][Mw]
 *           qzeros  int32 [K/gs][Mw*bits/32]   NULL exactly when cfg->zero_point == 0.  The blob's zero is T-MAC's,
 *                   (z + (gptq_v2 ? 0 : 1) - 2^(bits-1)) * scale: AutoGPTQ v1 stores z - 1.  The product is rounded ONCE, to scales_dtype,
 *                   then converted to ref_float -- numpy's result on the unpacked tensors, bit for bit (python/t_mac/model_utils.py:95-129)
 *           bits 1, 2, 4: the widths whose fields do not straddle a word.  bits = 3: TMAC_HIP_E_NOMATCH naming the width (use the codes form);
 *           m_groups >= 1: TMAC_HIP_E_ARG (GPTQ has per-group scales)
 *   codes   codes  uint8 [Mw][K], bits above `bits` ignored;  bits 1 .. 4
 *           scales, zeros  sz_dtype [Mw][K/gs], already in T-MAC's convention (zero = (z - 2^(bits-1)) * scale): copied and permuted only;
 *                   zeros NULL exactly when the configuration has no zero points.  m_groups >= 1: scales is [m_groups], copied; zeros NULL
 * Outputs: A_ref uint8 [M/bm][K/4][bm/2] and scales_ref in ref_float, the two arguments of tmac_hip_register_weights[_dev] (layouts above).
 * tmac_hip_ref_blob_bytes gives their sizes; it is a pure host function (no device is touched).
 * Refusals.  Shape and configuration: those of registration, same codes and messages (bm, kfactor, group sizes ...).  TMAC_HIP_E_ARG with
 * a message naming the argument, nothing written: a NULL required pointer; ANY device pointer of these calls below 16-byte alignment (the
 * kernels load and store 16 bytes at a time; rows stay aligned because Mw is a multiple of 8 and K of 4); zeros / qzeros present with
 * zero_point == 0, or absent with it set; m_groups >= 1 through the GPTQ form; a dtype other than TMAC_F32 / TMAC_F16.
 * tmac_hip_pack_*_dev write the two halves into the caller's device buffers, asynchronously on `stream`; they allocate nothing.  They are
 * ordered behind the calling thread's deferred queue ("deferred launches" below).  Nothing outside [pointer, pointer + bytes) of either
 * output is written, nothing outside the inputs' extents is read (tests/test_gpu_pack.py holds them to both).
 * tmac_hip_register_weights_*_dev pack into temporaries of their own and hand them to the registration above: every layout variant
 * (tmac_hip_set_variant), fast-aggregation mode and the kept-reference case behave as there, and the handle is the one registration from
 * the host blob gives.  They allocate and synchronise the stream, like registration.
 * While a chain is being recorded all four run at once and are not recorded, as registration does.  None of them is for use inside a
 * stream capture. */
int32_t tmac_hip_ref_blob_bytes(int Mw, int K, int bits, const tmac_kcfg* cfg, tmac_dtype_t ref_float, size_t* a_bytes, size_t* s_bytes);
int32_t tmac_hip_pack_gptq_dev(const void* qweight, const void* scales, const void* qzeros, tmac_dtype_t scales_dtype, int gptq_v2,
                               int Mw, int K, int bits, const tmac_kcfg* cfg, void* A_ref_out, void* scales_ref_out,
                               tmac_dtype_t ref_float, void* stream);
int32_t tmac_hip_pack_codes_dev(const void* codes, const void* scales, const void* zeros, tmac_dtype_t sz_dtype,
                                int Mw, int K, int bits, const tmac_kcfg* cfg, void* A_ref_out, void* scales_ref_out,
                                tmac_dtype_t ref_float, void* stream);
int32_t tmac_hip_register_weights_gptq_dev(tmac_hip_weights** out, const void* qweight, const void* scales, const void* qzeros,
                                           tmac_dtype_t scales_dtype, int gptq_v2, int Mw, int K, int bits, const tmac_kcfg* cfg,
                                           tmac_dtype_t ref_float, tmac_dtype_t dev_float, void* stream);
int32_t tmac_hip_register_weights_codes_dev(tmac_hip_weights** out, const void* codes, const void* scales, const void* zeros,
                                            tmac_dtype_t sz_dtype, int Mw, int K, int bits, const tmac_kcfg* cfg,
                                            tmac_dtype_t ref_float, tmac_dtype_t dev_float, void* stream);

/* ---- AutoAWQ checkpoints (WQLinear_GEMM, quantization_config.version "gemm", 4 bits) ---------------------------------------------
 * A third input form of the device-side packing above.  AWQ packs eight WEIGHT ROWS per word, along the output axis, interleaved:
 *   qweight int32 [K][Mw/8]     field i (bits 4i .. 4i+3) of word (k, c) is the code of weight row 8c + ORDER[i] at column k,
 *                               ORDER = (0, 2, 4, 6, 1, 3, 5, 7); row 8c + j sits in field INV[j], INV = (0, 4, 1, 5, 2, 6, 3, 7).
 *                               The word 0x76543210 gives rows 8c .. 8c+7 the codes 0, 4, 1, 5, 2, 6, 3, 7.
 *   scales  scales_dtype [K/gs][Mw]
 *   qzeros  int32 [K/gs][Mw/8]  the same field order; NULL exactly when cfg->zero_point == 0.  w = (q - z) * s with the stored z as it
 *                               is (no + 1): the codes are T-MAC's, the blob's zero is (z - 8) * scale, rounded ONCE to scales_dtype,
 *                               then converted to ref_float -- numpy's result on convert.unpack_awq's tensors, bit for bit
 * The width is 4 and no argument: cfg must describe 4 bits (cfg->bm * cfg->n_tile_num == 4 * Mw where n_tile_num is filled in), anything
 * else is TMAC_HIP_E_ARG, "AWQ is packed at 4 bits".  k_pack_awq_weights (tmac_pack.hip) reads every qweight word once; 16-byte loads
 * where Mw is a multiple of 32 (every row of qweight then is 16-byte aligned), word loads otherwise.  The two calls are ordered behind
 * the calling thread's deferred queue, which comes first.  Refusals, nothing launched and nothing written: as for the GPTQ pair --
 * TMAC_HIP_E_ARG naming the argument for a NULL required pointer, any of the five base pointers below 16-byte alignment, qzeros present
 * with zero_point == 0 or absent with it set, m_groups >= 1, a dtype other than TMAC_F32 / TMAC_F16; shape and configuration refusals are
 * registration's own.  The handle is an ordinary per-group handle: tmac_hip_weights_set_bias_dev works on it unchanged.  Not served: the
 * GEMV, GEMV-fast and Marlin versions of the format, widths other than 4, bf16 scales. */
int32_t tmac_hip_pack_awq_dev(const void* qweight, const void* scales, const void* qzeros, tmac_dtype_t scales_dtype, int Mw, int K,
                              const tmac_kcfg* cfg, void* A_ref_out, void* scales_ref_out, tmac_dtype_t ref_float, void* stream);
int32_t tmac_hip_register_weights_awq_dev(tmac_hip_weights** out, const void* qweight, const void* scales, const void* qzeros,
                                          tmac_dtype_t scales_dtype, int Mw, int K, const tmac_kcfg* cfg, tmac_dtype_t ref_float,
                                          tmac_dtype_t dev_float, void* stream);

/* ---- BitNet b1.58 master weights: the absmean rule on the device ------------------------------------------------------------
 * A BitNet checkpoint from its authors holds no codes: it holds master weights W [Mw][K], row-major, in fp32, fp16 or bf16 (src_dtype; a
 * dtype of its own -- tmac_dtype_t keeps its two values and its refusals).  The ternary levels come from the absmean rule of the BitNet
 * b1.58 paper, applied here at load time.  The rows are divided into m_groups blocks of R = Mw / m_groups rows; for block g
 *   gamma_g = fp32(sum |fp64(w)| / (R K))      accumulated in fp64 (k_absmean: fixed chunks, no atomics, chunk sums added in index order:
 *                                              the same bits on every launch, stream and GPU)
 *   s_g     = fmaxf(gamma_g, eps)              the unified scale stored for the block; eps: finite, > 0 (the paper's and the authors' 1e-5f)
 *   t       = clamp(rintf(fp32(w) * (1.0f / s_g)), -1, 1)      every operation fp32 and correctly rounded, halves to even; a NaN gives 0
 *   level   = t + 2                            {-1, 0, 1} -> levels 1, 2, 3 of the 2-bit format (w_real = (level - 2) s_g), level 0 unused
 * The conversions of fp16 / bf16 masters to fp32 and of |w| to fp64 are exact.  scales_in_dev (fp32 [m_groups], device) hands in the s_g
 * themselves -- a scale computed elsewhere or one the checkpoint carries: the reduction is skipped and the values are used as they are;
 * keeping them > 0 is the caller's job.  NULL: computed.  Non-finite masters with a computed scale: an infinity makes its block's scale
 * +infinity (every level of the block is then 2), a NaN is dropped by fmaxf (s_g = eps); no address depends on either.
 *   tmac_hip_absmean_dev                   the reduction alone: s_g -> scales_out_dev (fp32 [m_groups]); K a multiple of 4
 *   tmac_hip_pack_absmean_dev              -> the reference blob (sizes: tmac_hip_ref_blob_bytes with bits = 2); the levels go straight into
 *                                          A_ref_out (k_pack_dense_weights: the codes kernel with a quantising stage 1 -- no [Mw][K] code
 *                                          tensor is written anywhere), the m_groups scales into scales_ref_out as host_float
 *   tmac_hip_register_weights_absmean_dev  packs into temporaries, then registers as tmac_hip_register_weights_codes_dev does
 * Scope: bits = 2, unified scales (cfg->m_groups >= 1, Mw a multiple of it), whatever else registration accepts for such a configuration.
 * Refusals, nothing launched and nothing written.  TMAC_HIP_E_ARG naming the argument: a NULL pointer (scales_in_dev excepted) or one below
 * 16-byte alignment; an unknown src_dtype; eps not finite or <= 0; m_groups < 1 (per-group scales: register codes or GPTQ tensors);
 * Mw % m_groups.  Shape refusals are registration's own codes and messages, as in tmac_hip_pack_codes_dev.
 * All three are ordered behind the calling thread's deferred queue: they flush it first, a refused call leaves it alone, a failed flush
 * returns its status and launches nothing.  The reduction needs scratch (8 bytes per 16384 masters), allocated and freed by the call: with
 * a computed scale a call waits for `stream` before it returns; with scales_in_dev the pack allocates nothing and is asynchronous. */
typedef enum { TMAC_SRC_F32 = 0, TMAC_SRC_F16 = 1, TMAC_SRC_BF16 = 2 } tmac_src_dtype_t;
int32_t tmac_hip_absmean_dev(const void* W_dev, tmac_src_dtype_t src_dtype, int Mw, int K, int m_groups, float eps, float* scales_out_dev,
                             void* stream);
int32_t tmac_hip_pack_absmean_dev(const void* W_dev, tmac_src_dtype_t src_dtype, const float* scales_in_dev /* NULL: computed */, float eps,
                                  int Mw, int K, const tmac_kcfg* cfg, void* A_ref_out, void* scales_ref_out, tmac_dtype_t host_float,
                                  void* stream);
int32_t tmac_hip_register_weights_absmean_dev(tmac_hip_weights** out, const void* W_dev, tmac_src_dtype_t src_dtype,
                                              const float* scales_in_dev /* NULL: computed */, float eps, int Mw, int K, const tmac_kcfg* cfg,
                                              tmac_dtype_t host_float, tmac_dtype_t dev_float, void* stream);

/* ---- BitNet b1.58 packed ternary checkpoints: four weight rows per byte, unpacked on the device --------------------------------
 * A checkpoint written by the Hugging Face BitNet quantiser (quant_method "bitnet", offline mode; microsoft/bitnet-b1.58-2B-4T) holds no
 * master weights: it holds the ternary levels, packed.  packed_dev is uint8 [Mw / 4][K], row-major.  With R4 = Mw / 4, weight row o lives in
 * packed row o % R4, in the 2-bit field o / R4 at bit 2 (o / R4): the four row blocks of the matrix share a byte.  The stored field is
 * v = t + 1, t in {-1, 0, 1}; the blob's 2-bit level is t + 2 = v + 1 (levels 1, 2, 3, w_real = (level - 2) s, as above).  v = 3 occurs in no
 * well-formed file and has no level: it is packed as level 3 (t = 2 clamped to 1) and COUNTED.
 * scales_dev: fp32 [cfg->m_groups] in device memory, the unified scale s of each block of Mw / m_groups rows, copied into the blob as
 * host_float.  A checkpoint carries one `weight_scale`; which s it means is the caller's to say (quantization_config.linear_class:
 * "autobitlinear" multiplies by it, s = weight_scale; "bitlinear" divides, s = 1.0f / weight_scale -- tmac_amd/convert.py:bitnet_packed_scale).
 *   tmac_hip_pack_ternary_dev              -> the reference blob (sizes: tmac_hip_ref_blob_bytes with bits = 2).  The levels go straight into
 *                                          A_ref_out: no [Mw][K] code tensor is written anywhere.  Where (Mw / 4) % 16 == 0 -- every matrix of
 *                                          the 2B-4T and 3B models -- k_pack_ternary_weights_x4 reads every packed byte once and writes the four
 *                                          output tiles it feeds; otherwise k_pack_ternary_weights, the codes kernel with an extracting stage 1,
 *                                          reads each byte from four tiles.  invalid_count_dev (device int32; NULL: not counted): zeroed on the
 *                                          stream, then the number of fields of value 3 is added to it, at most one atomicAdd per workgroup.
 *                                          Asynchronous on `stream`; allocates nothing.
 *   tmac_hip_register_weights_ternary_dev  packs into temporaries with a counter of its own, synchronises and reads the counter: non-zero is
 *                                          TMAC_HIP_E_ARG, "packed weight holds %d fields of value 3 (no ternary level)", and no handle;
 *                                          otherwise registers as tmac_hip_register_weights_codes_dev does.
 * Scope: bits = 2, unified scales (cfg->m_groups >= 1, Mw a multiple of it), whatever else registration accepts for such a configuration
 * (Mw is then a multiple of 16 and K of 32).
 * Refusals, nothing launched and nothing written.  TMAC_HIP_E_ARG naming the argument: a NULL pointer (invalid_count_dev excepted) or any
 * device pointer below 16-byte alignment, the counter's included; m_groups < 1 (per-group scales: register codes or GPTQ tensors);
 * Mw % m_groups; host_float / dev_float other than TMAC_F32 / TMAC_F16.  Shape refusals are registration's own codes and messages, as in
 * tmac_hip_pack_codes_dev.
 * Both are ordered behind the calling thread's deferred queue: they flush it first, a refused call leaves it alone, a failed flush returns
 * its status and launches nothing.  While a chain is being recorded both run at once and are not recorded, as registration does.
 * tmac_hip_debug_pack_ternary_kernel: 0 (default) the read-once kernel where it applies; 1 the general form everywhere (tests, A/B).
 * tmac_hip_reset_state puts it back to 0. */
int32_t tmac_hip_pack_ternary_dev(const void* packed_dev, const float* scales_dev /* fp32 [m_groups] */, int Mw, int K, const tmac_kcfg* cfg,
                                  void* A_ref_out, void* scales_ref_out, tmac_dtype_t host_float, int32_t* invalid_count_dev /* NULL: not counted */,
                                  void* stream);
int32_t tmac_hip_register_weights_ternary_dev(tmac_hip_weights** out, const void* packed_dev, const float* scales_dev, int Mw, int K,
                                              const tmac_kcfg* cfg, tmac_dtype_t host_float, tmac_dtype_t dev_float, void* stream);
int32_t tmac_hip_debug_pack_ternary_kernel(int mode);

/* ---- dense master weights to W1 - W4 with per-group scales: round to nearest on the device -----------------------------------
 * An unquantised model holds W [Mw][K], row-major, in fp32, fp16 or bf16 (src_dtype, as above).  The codes and the per-group scales come
 * from GPTQ's quantiser without the error search (Quantizer.find_params with mse = False, then quantize), applied here at load time.  For
 * weight row o and group sg of group_size consecutive k, maxq = 2^bits - 1, every step one correctly rounded fp32 operation:
 *   lo = min(min_k w, 0), hi = max(max_k w, 0)
 *   without zero points (cfg->zero_point == 0):  hi = max(|lo|, hi), lo = -hi, zq = 2^(bits-1)
 *   scale = (hi - lo) / maxq;    lo == hi == 0, or scale below the smallest normal fp32:  lo = -1, hi = +1
 *   scale_f16:  scale = fp16(scale) -- the scale that divides is the scale that is stored
 *   with zero points:  zq = rint(-lo / scale)                       halves to even
 *   code = clamp(rint(w / scale) + zq, 0, maxq);   T-MAC's zero = (zq - 2^(bits-1)) * scale, so |w - w_real| <= scale / 2
 * A group is INVALID when a master of it is not finite, or when its scale is 0 or not finite (an fp16 scale that under- or overflowed): it
 * gets the parameters of the all-zero group, a NaN master code 0, and it is COUNTED.
 *   tmac_hip_rtn_params_dev            scale and zq of every (row, group) -> scales_out_dev / zq_out_dev, fp32 [Mw][K / group_size] each;
 *                                      group_size a multiple of 4 that divides K.  invalid_count_dev (device int32; NULL: not counted):
 *                                      zeroed on the stream, then the number of invalid groups is added to it, at most one atomicAdd per
 *                                      workgroup.  Asynchronous on `stream`; allocates nothing.
 *   tmac_hip_pack_rtn_dev              -> the reference blob (sizes: tmac_hip_ref_blob_bytes): k_rtn_params into scratch of the call's own
 *                                      (12 bytes per group), then the codes straight into A_ref_out (k_pack_rtn_weights: the codes kernel
 *                                      with a quantising stage 1 -- no [Mw][K] code tensor is written anywhere) and scales and zeros into
 *                                      scales_ref_out as host_float.  scale_f16 is host_float == TMAC_F16.  Invalid groups are counted as
 *                                      above, not refused.  Waits for `stream` before it returns (the scratch goes with the call).
 *   tmac_hip_register_weights_rtn_dev  packs into temporaries with a counter of its own (scale_f16 where host_float or dev_float is
 *                                      TMAC_F16), reads the counter: non-zero is TMAC_HIP_E_ARG, "master weights hold %d groups that cannot
 *                                      be quantised ...", and no handle; otherwise registers as tmac_hip_register_weights_codes_dev does.
 *                                      The handle is the one that call gives for the codes, scales and zeros of the rule.
 * Scope: bits 1 to 4, per-group scales (cfg->m_groups < 1), with or without zero points, whatever else registration accepts.
 * Refusals, nothing launched and nothing written.  TMAC_HIP_E_ARG naming the argument: a NULL pointer (invalid_count_dev excepted) or one
 * below 16-byte alignment; an unknown src_dtype; m_groups >= 1 (unified scales from master weights: tmac_hip_register_weights_absmean_dev);
 * host_float / dev_float other than TMAC_F32 / TMAC_F16; for the parameters alone, bits outside 1 to 4 or a group_size that is no positive
 * multiple of 4 dividing K.  Shape refusals of the two that pack are registration's own, code and message.
 * All three are ordered behind the calling thread's deferred queue: they flush it first, a refused call leaves it alone, a failed flush
 * returns its status and launches nothing. */
int32_t tmac_hip_rtn_params_dev(const void* W_dev, tmac_src_dtype_t src_dtype, int Mw, int K, int bits, int group_size, int zero_point, int scale_f16,
                                float* scales_out_dev, float* zq_out_dev, int32_t* invalid_count_dev /* NULL: not counted */, void* stream);
int32_t tmac_hip_pack_rtn_dev(const void* W_dev, tmac_src_dtype_t src_dtype, int Mw, int K, int bits, const tmac_kcfg* cfg, void* A_ref_out,
                              void* scales_ref_out, tmac_dtype_t host_float, int32_t* invalid_count_dev /* NULL: not counted */, void* stream);
int32_t tmac_hip_register_weights_rtn_dev(tmac_hip_weights** out, const void* W_dev, tmac_src_dtype_t src_dtype, int Mw, int K, int bits,
                                          const tmac_kcfg* cfg, tmac_dtype_t host_float, tmac_dtype_t dev_float, void* stream);

/* ---- act-order (desc_act) GPTQ matrices: the K permutation ---------------------------------------------------------------
 * An act-order matrix is a group-quantised matrix whose K axis is permuted: g_idx[k] names the group of column k.  With
 * perm = stable_argsort(g_idx) the columns q[:, perm] lie in contiguous groups of group_size, scales / qzeros are in group order already,
 * and y = W x = W' x[perm].  The handle holds W'; every LUT build that serves it reads its activations through perm.
 *
 * tmac_hip_kperm_from_gidx_dev  g_idx_dev: int32 [K] in device memory, 16-byte aligned.  One device-to-host copy, a stable counting sort
 *   on the host, one upload of perm (int32 [K]); synchronises the stream.  Ordered behind the calling thread's deferred queue.  Refused
 *   with TMAC_HIP_E_ARG and a message naming the first offending group, nothing created: a NULL or misaligned pointer, K % group_size != 0,
 *   a value outside [0, K / group_size), a group without exactly group_size members.  After success every perm[k'] < K, which keeps every
 *   device gather inside its row.
 * tmac_hip_kperm_info   K; identity = 1 when perm[k'] == k' throughout (g_idx == k / group_size, what every non-act-order exporter writes);
 *   id = a 64-bit hash of the contents, never 0.  Any out pointer may be NULL.
 * tmac_hip_kperm_read   the K values of perm to host memory.
 * tmac_hip_kperm_free   releases the caller's reference; handles registered through the object keep it alive.
 * Two objects are the same permutation when they are one object or K, hash and contents (memcmp) are equal.
 *
 * Packing and registration through a permutation take the argument lists of their plain twins plus `perm` behind the inputs.  perm NULL
 * or an identity: the plain twin is called.  Otherwise the twin's argument rules apply, and TMAC_HIP_E_ARG for: the permutation's K or
 * group size differing from the call's K / cfg->group_size; unified scales (m_groups >= 1).  The blob (tmac_hip_pack_*_perm_dev) is bit
 * for bit the plain pack's of the matrix with its columns gathered, w[:, perm]; scales and zeros are the plain pack's.  The registered
 * handle carries the permutation (tmac_hip_weights_kperm_id: its id, 0 for a plain handle).
 *
 * What serves such handles: tmac_hip_qgemm_fused_dev -- all matrices of a call must carry the same permutation, or none ("matrices fused
 * in one launch must share the K permutation", TMAC_HIP_E_ARG); N = 1 runs k_gemv_quad's gather instantiations, N >= 2 is routed as
 * tmac_hip_qgemm_fused_xf_rows_dev routes a transformed call with the LUT build gathering; QUAD layout and the MFMA accumulate only
 * (TMAC_HIP_E_NOMATCH otherwise).  The call is never queued (deferred mode: it goes behind the queue and launches stand-alone).  Between
 * tmac_hip_chain_begin and _end it is refused (TMAC_HIP_E_ARG; the recording stays usable): such a recording may end as k_decode_chain,
 * which has no gather.  A recording that was DECLARED INDEPENDENT (tmac_hip_chain_begin_independent, below) notes it (N = 1): that
 * recording can only become stream mode, whose LUT build (k_lut_images) gathers x[perm] per call; k_gemv_stream sees finished tables, so
 * the launch is the one the plain twins W[:, perm] on x[perm] get, bit for bit.  The chain keeps its calls' permutations alive.  The split path:
 * tmac_hip_preprocessor_perm_dev + tmac_hip_qgemm_dev, below.  Refused with TMAC_HIP_E_ARG and a message: the parity taps of the fused
 * entry point (tmac_hip_qgemm_fused_partial_sums) and vector transforms (tmac_hip_qgemm_fused_xf_dev, _xf_rows_dev) on such handles. */
typedef struct tmac_hip_kperm tmac_hip_kperm;
int32_t tmac_hip_kperm_from_gidx_dev(const int32_t* g_idx_dev, int K, int group_size, tmac_hip_kperm** out, void* stream);
int32_t tmac_hip_kperm_info(const tmac_hip_kperm* p, int* K, int* identity, uint64_t* id);
int32_t tmac_hip_kperm_read(const tmac_hip_kperm* p, int32_t* perm_host);     /* K values */
int32_t tmac_hip_kperm_free(tmac_hip_kperm* p);                               /* handles that use it keep it alive */
int32_t tmac_hip_weights_kperm_id(const tmac_hip_weights* w, uint64_t* id);   /* 0: the handle carries no permutation */
int32_t tmac_hip_pack_gptq_perm_dev(const void* qweight, const void* scales, const void* qzeros, tmac_dtype_t scales_dtype, int gptq_v2,
                                    const tmac_hip_kperm* perm, int Mw, int K, int bits, const tmac_kcfg* cfg, void* A_ref_out,
                                    void* scales_ref_out, tmac_dtype_t ref_float, void* stream);
int32_t tmac_hip_pack_codes_perm_dev(const void* codes, const void* scales, const void* zeros, tmac_dtype_t sz_dtype,
                                     const tmac_hip_kperm* perm, int Mw, int K, int bits, const tmac_kcfg* cfg, void* A_ref_out,
                                     void* scales_ref_out, tmac_dtype_t ref_float, void* stream);
int32_t tmac_hip_register_weights_gptq_perm_dev(tmac_hip_weights** out, const void* qweight, const void* scales, const void* qzeros,
                                                tmac_dtype_t scales_dtype, int gptq_v2, const tmac_hip_kperm* perm, int Mw, int K, int bits,
                                                const tmac_kcfg* cfg, tmac_dtype_t ref_float, tmac_dtype_t dev_float, void* stream);
int32_t tmac_hip_register_weights_codes_perm_dev(tmac_hip_weights** out, const void* codes, const void* scales, const void* zeros,
                                                 tmac_dtype_t sz_dtype, const tmac_hip_kperm* perm, int Mw, int K, int bits,
                                                 const tmac_kcfg* cfg, tmac_dtype_t ref_float, tmac_dtype_t dev_float, void* stream);

/* ---- biased linear layers: y = W x + b -------------------------------------------------------------------------------------
 * tmac_hip_weights_set_bias_dev gives a registered handle a bias: bias_dev is [Mw] of dtype F32, F16 or BF16 in device memory, 16-byte
 * aligned.  The handle owns an fp32 copy (the conversions are exact; padded with zeros to a multiple of 64 elements, so that a 16-byte
 * load at a tile's edge reads the library's own zeros); the call flushes the calling thread's deferred queue first and returns with the
 * copy made: the caller's buffer is free for reuse once `stream` is synchronised.  tmac_hip_free_weights frees the copy.  Set once,
 * straight after registration: a chain recorded earlier on the handle (and a launch of it) does not see the bias.
 * From then on every call on the handle computes y = W x + b: the bias is added to the fp32 output value in front of its one store -- one
 * correctly rounded add (rn), so a biased call equals rn(plain call's fp32 value + b) bit for bit, and its fp16 output is that sum rounded
 * once.  Two kernels carry the add: k_gemv_quad's MFMA form and k_gemm_planes' per-group flavour.  tmac_hip_qgemm_fused_dev (one call may mix
 * biased and plain matrices) and tmac_hip_qgemm_dev take the plan the plain call takes and are refused with TMAC_HIP_E_NOMATCH, naming the
 * route, before the first launch where it lands on another kernel (k_gemm_onehot, k_gemv_rows forced, variants 3 and 7, ...).
 * tmac_hip_qgemm_fused_xf_dev / _xf_rows_dev: TMAC_XF_NORM and the silu GLU are served; TMAC_XF_GLU_NORM and the relu^2 / GELU gates in
 * front of a biased matrix are refused with TMAC_HIP_E_NOMATCH at every N.  A call with a biased matrix is never recorded (refused with
 * TMAC_HIP_E_ARG, "carries a bias", in plain and declared-independent recordings alike; the recording stays usable), never queued (it
 * runs behind the deferred queue, stand-alone) and never tapped (TMAC_HIP_E_ARG).
 * Refused with a message, the handle unchanged: a NULL or misaligned bias_dev, a dtype outside the three, a handle that already has a bias,
 * a handle that carries a K permutation (TMAC_HIP_E_ARG); unified-scale handles, and handles outside the QUAD layout, with fast
 * aggregation or of a shape k_gemv_quad does not take (TMAC_HIP_E_NOMATCH). */
int32_t tmac_hip_weights_set_bias_dev(tmac_hip_weights* w, const void* bias_dev, tmac_src_dtype_t dtype, void* stream);
int32_t tmac_hip_weights_has_bias(const tmac_hip_weights* w, int* has);

/* LUT workspace = TMACGeMMWrapper::set_workspace (tmac_gemm_wrapper.h:257-270) on the device. */
int32_t tmac_hip_workspace_create(tmac_hip_workspace** out, int maxK, int maxN);
int32_t tmac_hip_workspace_free(tmac_hip_workspace* ws);

/* preprocessor (lut_ctor.cc:38-266 + generated glue): activations B_dev [N][K] (act_dtype) ->
 * ws {QLUT int8, lut_scales, lut_biases}.  Bit-exact with the reference's fp32 arithmetic.  B_dev: 16-byte aligned. */
int32_t tmac_hip_preprocessor_dev(tmac_hip_workspace* ws, const void* B_dev, tmac_dtype_t act_dtype,
                                  int K, int N, int act_group_size, void* stream);

/* The same through a K permutation (act-order handles, above): every layout of the workspace from B_dev[:, perm], by the gathered
 * pair-wise build, for every N; act_group_size must be 64 (TMAC_HIP_E_NOMATCH otherwise) and the permutation's K the call's
 * (TMAC_HIP_E_ARG).  The workspace records the id of the permutation its LUT was built through -- 0 for none, which every other build
 * and tmac_hip_workspace_write set.  perm NULL or an identity: tmac_hip_preprocessor_dev itself. */
int32_t tmac_hip_preprocessor_perm_dev(tmac_hip_workspace* ws, const void* B_dev, tmac_dtype_t act_dtype,
                                       int K, int N, int act_group_size, const tmac_hip_kperm* perm, void* stream);

/* qgemm_lut (tbl.cc + glue): C_dev [N][Mw] (out_dtype) = W x LUT(ws).  ws must hold the LUT of the
 * same K and act_group_size.  Whole matrix in one launch.  C_dev: 16-byte aligned (fp32), 8-byte (fp16).
 * TMAC_HIP_E_ARG when the weights carry a K permutation and the workspace's LUT was not built through it, or the reverse. */
int32_t tmac_hip_qgemm_dev(const tmac_hip_weights* w, const tmac_hip_workspace* ws, void* C_dev,
                           tmac_dtype_t out_dtype, int N, void* stream);

/* Fused form of llama_cpp_init + llama_cpp_compute (tmac_gemm_wrapper.h:170-228) for up to 4 weight
 * matrices that consume the SAME activation rows (q/k/v, gate/up): the LUT is built inside the GEMV
 * kernel (bit-exact with tmac_hip_preprocessor_dev) and every matrix is covered by one launch.
 *   weights[i] : registered matrices sharing K, bits and quantisation config
 *   B_dev      : activations [N][K] (act_dtype);   C_dev[i] : [N][Mw_i] (out_dtype)
 *   B_dev 16-byte aligned, every C_dev[i] 16-byte (fp32) or 8-byte (fp16) aligned ("Alignment" above)
 * With N at or above the GEMM threshold (tmac_hip_set_gemm_min_n) the call runs the preprocessor once into a
 * library-owned, per-stream workspace and the one-hot MFMA GEMM per matrix; the workspace is allocated on first use
 * (call once outside any stream capture) and released by tmac_hip_cache_clear().  The same workspace, under the same rule, is used
 * from N = 2 on where the rows kernel (k_gemv_rows, tmac_hip_debug_rows_kernel) serves the call. */
int32_t tmac_hip_qgemm_fused_dev(const tmac_hip_weights* const* weights, int nmat, const void* B_dev,
                                 tmac_dtype_t act_dtype, void* const* C_dev, tmac_dtype_t out_dtype, int N,
                                 void* stream);

/* ---- deferred launches ---------------------------------------------------------------------
 * For callers that do not record (a backend hook called mat-mul by mat-mul).  tmac_hip_defer(1): from now on the calling thread's N = 1
 * tmac_hip_qgemm_fused_dev calls are QUEUED instead of launched; tmac_hip_flush launches what is queued as ONE stream-mode launch
 * (k_lut_images + k_gemv_stream: the independent-call path, 0.6-0.75 of the HBM peak instead of 0.25 for stand-alone launches).  The
 * queue never holds a dependence: a call that reads, or overwrites, anything a queued call writes (or overwrites what one reads), a call on
 * another stream, an N > 1 call and tmac_hip_defer(0) flush it first -- results are those of launching the calls in order (per-group-scale
 * outputs of a batch to the tolerance of the stream kernel, not bit for bit: k_gemv_stream's default quarter-walk form adds a row's fp32
 * partial sums in another order than a stand-alone launch, see tmac_hip_chain_is_stream; integers and unified-scale outputs are the same).
 * EVERY other entry point that launches work or touches device memory for the caller is ordered behind the calling thread's queue too: it
 * flushes the queue first, unconditionally (no overlap analysis: none of them is a hot path) -- tmac_hip_preprocessor_dev,
 * tmac_hip_qgemm_dev, tmac_hip_qgemm_partial_sums, tmac_hip_qgemm_fused_partial_sums, tmac_hip_chain_launch, tmac_hip_workspace_read /
 * _write, tmac_hip_debug_gemm_comb_sums / _gemm_image_read, tmac_hip_autotune_fused, tmac_hip_pack_gptq_dev / _pack_codes_dev (they write the
 * caller's blob buffers; a refused one leaves the queue alone), tmac_hip_absmean_dev / _pack_absmean_dev /
 * _register_weights_absmean_dev (the same), tmac_hip_pack_ternary_dev / _register_weights_ternary_dev (the same), tmac_hip_rtn_params_dev / _pack_rtn_dev /
 * _register_weights_rtn_dev (the same), and tmac_hip_free_weights, tmac_hip_chain_free and
 * tmac_hip_cache_clear (a queued call may name what they release).  When that flush fails the entry point returns its status and launches
 * nothing of its own (the three that release still release: the handle is dead either way).  A queue belongs to a thread: freeing, from
 * another thread, weights that this thread has queued is the caller's error.
 * A call is checked when it is queued: one that would be refused with deferral off is refused at once with the same code and message, is
 * not queued and leaves the queue alone.  A flush launches EVERY queued call whatever fails on the way -- after a failed stream launch
 * that group's calls one by one, after a failed call the rest -- returns the first error of a call that could not be launched, and leaves
 * the queue empty.  An N > 1 call whose flush fails returns that error and is not launched.  tmac_hip_defer(0) leaves deferred mode
 * whatever its flush returns; tmac_hip_reset_state ends with the mode off and the queue empty.
 * tmac_hip_flush launches the queue on the stream its calls were ISSUED on, whatever its argument.  The recording
 * built from a batch is cached by the batch's signature (matrices, pointers, dtypes; invalidated when weights are freed): a decode loop
 * pays for it once.  A batch that mixes configurations (bits, zero points, per-group / unified scales, scale or output dtype) becomes one
 * stream launch per configuration -- its calls are independent of each other; calls the persistent kernels do not cover, and configurations
 * with fewer than three calls (a stream launch costs ~10 us before its first byte), are launched one by one at the flush.  Group size is no
 * part of a configuration: a batch's calls of group size 64 join the stream launch of their configuration as those of 128 do, and that
 * launch then runs the two-scale-group instantiation (the results of its group-size >= 128 calls are bit-identical either way).  The caller must flush before it
 * synchronises the stream or reads an output.  tmac_hip_defer_stats: flushes, cache hits, stream-mode launches, calls launched singly.
 * The cached recordings of a thread are released by tmac_hip_cache_clear() / tmac_hip_reset_state() called on that thread. */
int32_t tmac_hip_defer(int on);
int32_t tmac_hip_flush(void* stream);
int32_t tmac_hip_defer_stats(uint64_t* flushes, uint64_t* cache_hits, uint64_t* stream_launches, uint64_t* single_calls);

/* ---- persistent decode chain ---------------------------------------------------------------
 * The fused calls of one decoded token (llama.cpp issues the same tmac_hip_qgemm_fused_dev sequence for every token:
 * llama_cpp_init + llama_cpp_compute per projection, tmac_gemm_wrapper.h:170-228) recorded ONCE and executed by ONE
 * persistent kernel launch (k_decode_chain): one workgroup per CU walks the whole list, weights of the next call stream in
 * while the current one computes, and an output that a later call takes as its activations is handed over inside the
 * launch (self-tagged fp16 granules, no kernel boundary).  Recording works like stream capture:
 *     tmac_hip_chain_begin();
 *     ... the thread's usual tmac_hip_qgemm_fused_dev(..., N = 1, ...) calls: noted, not launched ...
 *     tmac_hip_chain_end(&chain);
 *     tmac_hip_chain_launch(chain, stream);      // per token; outputs land in the C_dev buffers given while recording
 * Data flow is inferred from pointer identity: a call whose B_dev equals an earlier call's C_dev[i] consumes that output
 * inside the launch; any other B_dev must hold its activations when the launch starts.  Calls execute in recorded order.
 * An output buffer may be written by several calls (a decoder reuses its buffers layer after layer); the last one wins.
 * Scope: 1- to 4-bit QUAD-layout weights; per-group scales (group size >= 64, a power of two; the calls of a chain may differ in it)
 * with act groups of 64, or
 * unified scales (m_groups >= 1, BitNet) with one act group per row; fp16 activations, or fp32 for vectors that are in memory before the launch; chained outputs fp16; one weight
 * width, scale flavour, scale dtype and zero-point setting per chain.  Anything else: -1 from tmac_hip_chain_end and
 * the caller keeps launching the calls one by one.  Results are bit-identical to tmac_hip_qgemm_fused_dev with
 * the same threads per workgroup and waves per row quad (tmac_hip_debug_quad_config(tmac_hip_chain_threads(), wpq)).
 * A recording with a call of group size 64 runs the kernels' two-scale-group instantiation (a lane's two act groups of a lookup item
 * then lie in two scale groups); the results of its calls of group size >= 128 are bit-identical to those of a recording without one.
 * A chain must not be launched concurrently with itself; the GPU must be able to hold one workgroup per CU (true unless
 * other work occupies CUs for the whole duration: every wait inside the kernel is bounded and reports through
 * tmac_hip_chain_status instead of hanging). */
typedef struct tmac_hip_chain tmac_hip_chain;
int32_t tmac_hip_chain_begin(void);
/* A recording DECLARED INDEPENDENT when it begins: the caller states that no recorded call reads another's output.  It works like
 * tmac_hip_chain_begin (_end, _abort, the launch and the inspection calls are the same), and in return tmac_hip_chain_end builds a
 * STREAM-MODE chain (k_lut_images + k_gemv_stream, tmac_hip_chain_is_stream != 0) or fails -- never k_decode_chain.  Its failures are
 * TMAC_HIP_E_ARG with a message naming the first offending call: a call reads an earlier call's output (both are named), a call carries
 * a transform, an exchange step was recorded, the stream planner has no form for the calls, or TMAC_CHAIN_STREAM=0 is set; as after
 * every failed _end the recording is over and the thread launches calls again.  tmac_hip_chain_xform and tmac_hip_chain_record_gather
 * are refused at once inside it (TMAC_HIP_E_ARG; the recording stays usable).  Because it can only become a stream, calls on act-order
 * handles (above) are noted in it: all matrices of a call carry the same permutation or none; the calls of a chain may mix plain
 * handles and different permutations.  A chain without such a call launches exactly what a tmac_hip_chain_begin recording of the same
 * independent calls launches. */
int32_t tmac_hip_chain_begin_independent(void);
int32_t tmac_hip_chain_end(tmac_hip_chain** out);
/* ends the recording without building a chain (after an error while recording: the thread launches its calls again) */
int32_t tmac_hip_chain_abort(void);
int32_t tmac_hip_chain_launch(tmac_hip_chain* chain, void* stream);
/* after synchronising the stream: *error_word == 0 means every hand-off completed; otherwise (bit 31 | op << 8 | wave of
 * the first wave that gave up) the outputs of that launch are invalid.  Clears the word and re-arms the chain. */
int32_t tmac_hip_chain_status(tmac_hip_chain* chain, uint32_t* error_word);
/* number of recorded calls, waves per row quad chosen for call `op`, workgroups, weight + scale bytes one launch streams
 * (any pointer may be NULL) */
int32_t tmac_hip_chain_info(const tmac_hip_chain* chain, int op, int32_t* nops, int32_t* wpq, int32_t* grid, size_t* bytes);
int32_t tmac_hip_chain_free(tmac_hip_chain* chain);
/* Vector transforms inside the chain.  Between two mpGEMMs of a decoder layer sit element-wise operators the hot path does not own
 * (residual add + RMSNorm in front of q/k/v and gate/up, gate(gate) * up in front of the down projection); as kernels of their own they
 * would end the persistent launch after every call.  Every workgroup of the chain holds a call's whole activation vector when it builds
 * the LUT, so these operators are applied THERE: tmac_hip_chain_xform, while recording, describes a transform of the activations of the
 * NEXT recorded tmac_hip_qgemm_fused_dev call (B_dev = `in`).  fp32 arithmetic; the LUT is built from the fp32 result.
 *   TMAC_XF_NORM  t = in + residual;  x = gamma ? t * (1 / sqrt(mean(t^2) + eps)) * gamma : t
 *                 residual: fp32 [K] in device memory, NULL (none), or TMAC_XF_CARRY = the t that the latest NORM with keep != 0 kept
 *                 (inside the launch, no memory round trip; K <= 8192); residual_out: t also goes to memory (fp32 [K], e.g. the residual
 *                 stream for the next launch).  tmac_hip_chain_end checks it like every other write of the launch: it may overlap a
 *                 vector an EARLIER call of the chain reads from memory only when a hand-off path from a call in which every workgroup
 *                 owns rows leads to this one (the in-place residual stream of a decoder segment); never the vectors this or a later
 *                 call reads (a later NORM takes TMAC_XF_CARRY), never an output
 *   TMAC_XF_GLU   x = gate(in) * in2;  in2: fp16 [K], an earlier output of the chain (handed over like `in`) or external memory -- of the
 *                 same kind as `in`; K <= 12288.  gate: silu unless bits 8..15 of `kind` name another (TMAC_XF_GATE_*, below)
 *                 (when `in` and `in2` are outputs 0 and 1 of one earlier two-matrix call of the chain and nothing else reads output 0 through a
 *                 hand-off, that call publishes gate(in) * in2 itself, once per row, rounded to fp16 like every handed-over vector)
 *   TMAC_XF_GLU_NORM  g = gate(in) * in2;  x = g * (1 / sqrt(mean(g^2) + eps)) * gamma -- the sub-layer norm BitNet b1.58 puts between
 *                 gate(gate) * up and the down projection (ffn_sub_norm; silu in the 3B checkpoints, relu^2 in 2B-4T).  in2 as for a GLU;
 *                 gamma (fp32 [K]) is required; residual,
 *                 residual_out and keep must be NULL / 0 (TMAC_HIP_E_ARG names the field).  Recorded in the PRODUCER FORM ONLY: `in` and
 *                 `in2` are outputs 0 and 1 of one earlier two-matrix call that publishes gate(in) * in2 itself (the rule in brackets
 *                 above), and this call is then a NORM without residual of that handed-over vector; K <= 12288.  Every other form --
 *                 vectors in memory, gate and up from two calls, a gathered output, TMAC_CHAIN_GLU_EPILOGUE=0, a waves-per-quad choice
 *                 that cannot deal row pairs -- is TMAC_HIP_E_NOMATCH from tmac_hip_chain_end: issue the calls one by one
 * A decoder then runs one launch per segment between two operators that stay outside (attention): o -> gate/up -> down -> next q/k/v.
 * These are extensions without a reference counterpart (T-MAC has no norm operator): tests compare them with the same formulas in
 * numpy fed through the oracle (tolerance, not bits: the mean square is summed in another order).
 * EVERY RECORDING HAS A CALL-BY-CALL EQUIVALENT: "-1 from tmac_hip_chain_end, keep launching the calls one by one" holds for recordings
 * with transforms too -- a recorded call that carries one is tmac_hip_qgemm_fused_xf_dev (below) outside the recording.  That is what a
 * caller issues when tmac_hip_chain_end refuses the recording (LDS beyond 160 KB, K beyond the limits above, ...) or tmac_hip_chain_status
 * reports invalid outputs; two things do not carry over, because nothing outlives a stand-alone launch: a kept t (TMAC_XF_CARRY) is read
 * from the memory an earlier call wrote as residual_out, and an in-place residual stream alternates between two buffers (see there).
 * tmac_hip_chain_launch itself falls back to nothing.  A transform declared in front of a call that is rejected is dropped with it.
 * in2, residual (unless TMAC_XF_CARRY), gamma and residual_out are 16-byte aligned; a transform naming a vector that is not is refused with
 * TMAC_HIP_E_ARG and declares nothing.
 * THE GATE of a GLU / GLU_NORM travels in bits 8..15 of `kind`; the low byte is the kind.  kind = TMAC_XF_GLU_NORM | TMAC_XF_GATE_RELU2
 * reads g = relu(in)^2 * in2, then the sub-norm (BitNet b1.58 2B-4T's FFN); TMAC_XF_GLU | TMAC_XF_GATE_GELU is a GeGLU.  fp32:
 *   silu   v / (1 + exp(-v)), hardware exp and reciprocal: specified to a tolerance
 *   relu2  m = max(v, 0);  g = (m * m) * in2, each product rounded to nearest: exact arithmetic, specified to the bit
 *   gelu   the tanh form, written as the silu expression with z = 1.5957691216 v (1 + 0.044715 v^2) inside the exponential
 *          (0.5 (1 + tanh y) = 1 / (1 + exp(-2 y))): specified to a tolerance like silu
 * Refused with TMAC_HIP_E_ARG and a message naming the gate, by the one check tmac_hip_chain_xform, tmac_hip_qgemm_fused_xf_dev and
 * tmac_hip_qgemm_fused_xf_rows_dev share: gate bits on TMAC_XF_NONE or TMAC_XF_NORM, a gate value other than the three, any bit above 15.
 * (A low byte that is no kind -- 3, whatever the gate -- stays "unknown transform kind".)  The gate changes no rule above: routes, limits
 * and the producer form are those of the kind. */
#define TMAC_XF_NONE 0
#define TMAC_XF_NORM 1
#define TMAC_XF_GLU 2
#define TMAC_XF_GLU_NORM 4   /* (3 is not a kind) */
#define TMAC_XF_GATE_SILU  0x000   /* v / (1 + exp(-v))                                   (the default) */
#define TMAC_XF_GATE_RELU2 0x100   /* max(v, 0)^2                                                       */
#define TMAC_XF_GATE_GELU  0x200   /* tanh form: v / (1 + exp(-z)),  z = 1.5957691216f * v * (1 + 0.044715f * v * v) */
#define TMAC_XF_CARRY ((const float*)1)
typedef struct {
    int32_t kind;
    const void* in2;
    const float* residual;
    const float* gamma;
    float eps;
    float* residual_out;
    int32_t keep;
} tmac_hip_xform;
int32_t tmac_hip_chain_xform(const tmac_hip_xform* xf);
/* The stand-alone form: tmac_hip_qgemm_fused_dev(..., N = 1, ...) with the transform `xf` applied to its activations (B_dev = `in`) inside
 * the kernel, between the activation loads and the table build of k_gemv_quad -- every workgroup holds the whole vector there.  All
 * matrices of the call consume the same transformed vector (q/k/v, or gate/up, behind one NORM).
 *   xf == NULL or kind TMAC_XF_NONE   tmac_hip_qgemm_fused_dev(..., N = 1, ...) itself: same route, same kernel, same bits
 *   TMAC_XF_NORM   t = fp32(in) + residual (fp32 [K]; NULL: t = in);  x = gamma ? t * (1 / sqrt(mean(t^2) + eps)) * gamma : t.  fp32 rn adds; the
 *                  LUT is built from the fp32 x by the code of the plain call, so without gamma the outputs are those of a plain call on t,
 *                  bit for bit.  residual_out (fp32 [K], optional) receives t: each element is written once, pair p (8 elements) by
 *                  workgroup p mod grid.  `keep` is accepted and ignored; residual == TMAC_XF_CARRY is refused (TMAC_HIP_E_ARG)
 *   TMAC_XF_GLU    x = gate(in) * in2;  in2 has act_dtype like `in` (fp16 or fp32); silu and gelu: hardware exp and reciprocal, specified
 *                  to a tolerance; relu2: exact, (max(in, 0) * max(in, 0)) * in2 to the bit (TMAC_XF_GATE_* above)
 *   TMAC_XF_GLU_NORM  g = gate(in) * in2, the GLU's expression;  x = (g * gamma) * rsq(fma(sum g^2, rcp(K), eps)), the NORM's association
 *                  and reduction.  gamma is required; residual, residual_out and keep must be NULL / 0
 * Scope: what tmac_hip_qgemm_fused_dev serves with k_gemv_quad at N = 1 -- QUAD layout, 1- to 4-bit, per-group scales (group size >= 64,
 * act groups of 64) or unified scales (m_groups >= 1), MFMA accumulate -- for K up to 24576, the kernel's own limit (the transformed
 * vector stays in registers, no LDS is added).  Anything else: TMAC_HIP_E_NOMATCH, nothing is launched.
 * Refused with TMAC_HIP_E_ARG before anything is launched: a kind (low byte) other than 0, 1, 2, 4; gate bits (8..15) on kind 0 or 1, a gate
 * other than TMAC_XF_GATE_SILU / _RELU2 / _GELU, any bit above 15 (the message names the gate); GLU without in2; GLU_NORM without in2 or gamma, or
 * with residual, residual_out or keep set (the message names the field); in2 / residual / gamma / residual_out
 * not 16-byte aligned (B_dev and C_dev[i] as everywhere); residual_out overlapping B_dev, residual, gamma or a C_dev[i] -- every
 * workgroup reads the whole of the inputs while one workgroup writes each pair of residual_out, so an in-place residual stream has no
 * order here: alternate between two buffers.
 * While the thread records a chain the call is tmac_hip_chain_xform(xf) followed by the recorded tmac_hip_qgemm_fused_dev -- one call site
 * for both modes, the chain's rules apply there.  With deferral on a transformed call is never queued: it flushes the queue, then
 * launches (a failed flush returns its status and nothing is launched).
 * Launch configuration: tmac_hip_debug_quad_config and the tuned table are honoured; the transformed instantiations exist for (threads,
 * waves per quad) = (512,1), (512,2), (768,3), (1024,4) -- once for NORM / GLU and once for GLU_NORM, each serving the three gates.  A forced configuration outside that set is TMAC_HIP_E_NOMATCH; a tuned or
 * heuristic choice outside it runs on the nearest member (same waves per quad with 512 threads; (1024,4) for K > 12288). */
int32_t tmac_hip_qgemm_fused_xf_dev(const tmac_hip_weights* const* weights, int nmat, const void* B_dev, tmac_dtype_t act_dtype,
                                    const tmac_hip_xform* xf, void* const* C_dev, tmac_dtype_t out_dtype, void* stream);
/* The same for N activation rows -- prefill, or a batch of 2-8 rows -- so that one call site serves every N with one formula.
 * Layouts: B_dev and in2 [N][K] in act_dtype; residual and residual_out fp32 [N][K]; gamma fp32 [K], shared by the rows; C_dev[i]
 * [N][Mw_i] in out_dtype.  Row n of every operand belongs to row n of the activations.
 *   N = 1                             tmac_hip_qgemm_fused_xf_dev itself: same route, same kernel, same bits
 *   xf == NULL or kind TMAC_XF_NONE   tmac_hip_qgemm_fused_dev(..., N, ...) itself
 *   N >= 2   the call is planned like tmac_hip_qgemm_fused_dev(N) and the transform sits in the activation load of the planned LUT build
 *            (k_lut_image for k_gemm_planes, the pair builds for k_gemm_onehot / k_gemv_rows / the row loop): the LUT is built from the fp32
 *            x by the plain build's code, and the kernel behind it is the plain call's.  NORM with gamma or residual_out is preceded by
 *            one row pass (k_xf_rows, a workgroup per row) that writes residual_out -- every element once -- and the row's
 *            r = rsq(fma(sum t^2, rcp(K), eps)); the builders then form (t * gamma) * r.  GLU_NORM always takes the row pass: it sums g^2 in
 *            the same order and writes r alone; the builders recompute g with the row pass's own function (whatever the gate) and form
 *            (g * gamma) * r.
 *            The order of that sum depends on K alone: a row
 *            gives the same x whatever N, its index or the route.  (At N = 1 k_gemv_quad sums in its own order: the two forms agree to
 *            rounding, not bits, for NORM with gamma.)  Where the plain call would run k_gemv_quad with one LUT build per workgroup, the
 *            transformed call builds the half-table image once and runs the row loop on it.
 * Scope (N >= 2): QUAD layout, 1- to 4-bit, act groups of 64 or unified scales with K <= 12288, one configuration per call.
 * TMAC_HIP_E_NOMATCH, nothing launched: anything outside that scope, a plan that would need the three-layout LUT build, the
 * reference-layout variant, fast-aggregation weights.  TMAC_HIP_E_ARG, nothing launched: the refusals of the N = 1 form with extents
 * x N -- kind other than 0, 1, 2, 4, the gate's refusals, GLU without in2, GLU_NORM's own refusals, TMAC_XF_CARRY, a transform vector below 16-byte alignment, residual_out overlapping B_dev,
 * residual, gamma, in2 or an output (the LUT build reads `in` and `residual` after the row pass has written residual_out: alternate
 * between two buffers).
 * While the thread records a chain an N >= 2 transformed call is TMAC_HIP_E_NOMATCH: nothing is recorded, no transform stays pending.
 * With deferral on it is never queued: it flushes the queue (a failed flush returns its status, nothing is launched), then launches.
 * The row's r lives in the per-stream workspace of the fused entry point, allocated on first use: call once outside any stream capture.
 * in2 is ignored by a NORM except in the overlap rule above: a NORM whose struct still names an in2 that residual_out overlaps is
 * refused, where the N = 1 form does not look at it. */
int32_t tmac_hip_qgemm_fused_xf_rows_dev(const tmac_hip_weights* const* weights, int nmat, const void* B_dev, tmac_dtype_t act_dtype,
                                         const tmac_hip_xform* xf, void* const* C_dev, tmac_dtype_t out_dtype, int N, void* stream);
/* What the call above would run for N >= 2 rows on these matrices, under the current knobs (host only: plans, launches nothing):
 * route 0 k_gemm_planes, 1 k_gemm_onehot, 3 k_gemv_rows, 7 the row loop; lut 1 the LUT image, 2 the half-table image.  The planner's
 * refusals come back as from the call (the scope checks of the call itself are not repeated). */
int32_t tmac_hip_debug_xf_rows_plan(const tmac_hip_weights* const* weights, int nmat, void* const* C_dev, int N, int32_t* route, int32_t* lut);
/* What an untransformed tmac_hip_qgemm_fused_dev call of N >= 1 rows on these matrices would run, under the current knobs (host only:
 * plans, launches nothing).  route, in the order of the dispatcher's enum: 0 k_gemm_planes / k_gemm_planes_us, 1 k_gemm_onehot,
 * 2 k_gemv_quad (grid.y = N), 3 k_gemv_rows, 4 k_gemv_fused, 5 k_gemv_lo, 6 the reference-layout kernel, 7 the row loop (one LUT build,
 * then every matrix planned again as by tmac_hip_qgemm_dev).  lut, the build in front of the kernel: 0 none (the GEMV kernel builds its
 * own), 1 the LUT image, 2 the half-table image, 3 every layout of the workspace (tmac_hip_preprocessor_dev).  The planner's refusals
 * come back as from the call.  A recording, the deferred queue and a tap sit in front of the planner and are not modelled. */
int32_t tmac_hip_debug_fused_plan(const tmac_hip_weights* const* weights, int nmat, void* const* C_dev, int N, int32_t* route, int32_t* lut);
/* Launches per planned route since the library was loaded or reset (host counters, zeroed by tmac_hip_reset_state): counts[r] for the
 * route numbers above, r = 0 .. 7.  Counted where a planned route is launched -- tmac_hip_qgemm_dev and the host-pointer entry points
 * behind it, the fused entry point and its transformed forms -- so a row-loop call counts 1 under route 7 and, per matrix, 1 under the
 * route that matrix then took.  A call is counted when it is planned for launch, a tap's launch included; a recorded call is not
 * (a chain is no route), nor is a queued one that a flush serves from a chain.  Plain counters like tmac_hip_debug_rows_stats': exact
 * while one thread at a time makes calls. */
int32_t tmac_hip_debug_route_stats(uint64_t counts[8]);
/* Parity tap: the fp32 x [N][K] that the LUT builds of the call above consume (the row pass plus a store around the builders' own load;
 * residual_out is written as the call writes it).  kind NORM, GLU or GLU_NORM (the last two with any gate); argument rules as above; synchronises the stream. */
int32_t tmac_hip_debug_xf_rows(const void* B_dev, tmac_dtype_t act_dtype, const tmac_hip_xform* xf, int K, int N, float* x_out_dev,
                               void* stream);
/* Row-sharded chains (one process per GPU; weight ROWS split over the ranks).  While recording, the exchange step between
 * a call and the calls that need its output whole is recorded too -- tmac_hip_comm_allgather(comm, send, recv, ...) notes itself, or
 * tmac_hip_chain_record_gather where no communicator exists -- and inside the launch it becomes part of the hand-off: every rank's
 * producers store their granules into the hand-off arena of EVERY rank (IPC-mapped peer memory, system-scope stores over xGMI), the
 * consumers' polls are unchanged.  `recv` itself is NOT written by the launch.  Protocol, same recorded sequence on every rank:
 *     tmac_hip_chain_end(&chain);  tmac_hip_chain_export(chain, blob);          // TMAC_HIP_CHAIN_BLOB_BYTES
 *     ... all-gather the blobs over any transport (rank order) ...
 *     tmac_hip_chain_connect(chain, blobs_of_all_ranks, world);                 // hipIpcOpenMemHandle of the peers' arenas
 *     per token, on every rank: tmac_hip_chain_launch(chain, stream)            // the ranks' launches must overlap in time
 * K is never split, integer sums are those of one GPU.  HSA_ENABLE_IPC_MODE_LEGACY=0 must be set where the driver supports dmabuf IPC only. */
#define TMAC_HIP_CHAIN_BLOB_BYTES 128
int32_t tmac_hip_chain_record_gather(const void* send_dev, void* recv_dev, size_t bytes_per_rank, int rank, int world);
int32_t tmac_hip_chain_export(const tmac_hip_chain* chain, void* blob_out);
int32_t tmac_hip_chain_connect(tmac_hip_chain* chain, const void* blobs_of_all_ranks, int world);
int32_t tmac_hip_chain_threads(void);   /* threads per workgroup of k_decode_chain (the launch configuration its results are bit-identical with) */
/* Stream mode.  A recording in which NO call consumes another call's output (and none carries a transform) is a list of independent
 * GEMVs -- SURVEY 8(d)'s back-to-back measurement, or a caller that evaluates many vectors against many matrices.  tmac_hip_chain_end
 * then builds a different launch (1 = yes): k_lut_images builds the tables of every call ONCE -- the reference's own call structure,
 * llama_cpp_init per activation vector, then lookups only (tmac_gemm_wrapper.h:170-228) -- and k_gemv_stream walks the calls with the
 * tables prebuilt, a loader wave per workgroup staging the next call's tables while the lookup waves stream this call's weights; the
 * weight prefetch runs across call boundaries.  No hand-offs, no spins: residency is not a correctness condition there.  Since round 6
 * the calls are dealt to CLASSES of workgroups (a call that is small for 256 CUs is served by a fraction of them with more rows each,
 * other classes work on other calls meanwhile: TMAC_STREAM_NCLS=1 in the environment = every workgroup visits every call; further A/B
 * knobs read by tmac_hip_chain_end: TMAC_STREAM_VISIT_ITEMS (items a visit should give a workgroup, 160), TMAC_STREAM_LPT=0 (calls dealt in
 * recorded order instead of largest first), TMAC_STREAM_SPLIT=1 (one workgroup per CU), TMAC_STREAM_QW=0 | 1 (item form, below)).  Same integers
 * as every N = 1 path (tmac_hip_chain_set_tap); float outputs: see the return value 2 below.  Per-group scales, or unified scales
 * (BitNet: the row's scale and the sequential bias chain by k_lut_images_us, scale-final on exact int32 totals);
 * TMAC_CHAIN_STREAM=0 in the environment keeps the ordinary chain (A/B).  Group size >= 64: a stream with a call of group size 64 runs
 * the two-scale-group instantiation of k_gemv_stream (both forms); its calls of group size >= 128 give the bits they give in a stream
 * without one.  (3-bit streams with such a call keep one workgroup per CU.) */
/* Returns 0 (k_decode_chain), 1 (stream mode) or 2: stream mode in the QUARTER-WALK form -- rows dealt in groups of 16, K walked in quarters
 * of a 64-unit step, so that a K with a ragged last step (11008, 3200, 8640 ...) does not spend whole lookup items on zero tables.  Every
 * 1- or 2-bit stream whose matrices all have rows % 16 == 0 takes it (it is the faster form there even without a ragged step); a 3- or
 * 4-bit stream only when it also saves more than 15 % of the lookup items.  Same integers (tmac_hip_chain_set_tap shows them); a row's fp32 partial sums are added in another order than the stand-alone
 * launch adds them, so per-group-scale outputs are specified to the path's tolerance (<= 1e-3 of the reference, measured <= 2e-5) instead
 * of bit-identical to that launch; unified-scale outputs stay bit-identical.  TMAC_STREAM_QW=0 in the environment keeps form 1 (A/B). */
int32_t tmac_hip_chain_is_stream(const tmac_hip_chain* chain);
/* profiling / A-B knobs: s_memrealtime stamps (100 MHz) [calls][workgroups][8] of wave 0 (0 call entry, 1 activations complete, 2 LUT
 * built, 3 weights of the call landed, 5 last row quad published, 6 all loads landed, 7 number of polls) into a device buffer (NULL = off); waves per row quad forced for chains built from now on (0 = per-call
 * choice) and the poll limit of a hand-off (0 = keep).  The stamps exist in profiling builds of the library only (-DTMAC_CHAIN_STAMPS=1 for
 * k_decode_chain, -DTMAC_STREAM_STAMPS for k_gemv_stream: the idle hooks cost the dependent token 3 %); otherwise a non-NULL buffer returns -1 */
int32_t tmac_hip_chain_set_stamps(tmac_hip_chain* chain, unsigned long long* dev_buffer);
/* Parity tap of the persistent kernels (k_decode_chain, k_gemv_stream): the INTEGERS of every recorded call as they enter the float part of
 * the path, written by the launch itself into a caller's device buffer (NULL = off; launches with a tap run the kernels' tap instantiation).
 * Call `op` owns ints [offset, offset + count) (tmac_hip_chain_tap_layout; op == number of calls: offset = size of the whole buffer):
 * per-group scales: int32 [rows of the call's matrices, concatenated][K / 64] = sum_p 2^p PS_p per (weight row, act group), PS_p the
 * per-plane partial sums of tbl.cc:445-462 (what tmac_hip_qgemm_partial_sums returns per plane); unified scales: int32 [rows][bits], the
 * exact per-plane totals of tbl.cc:586-628.  Not available for calls whose rows are dealt in gate / up pairs (GLU in the producer). */
int32_t tmac_hip_chain_set_tap(tmac_hip_chain* chain, int32_t* dev_buffer);
int32_t tmac_hip_chain_tap_layout(const tmac_hip_chain* chain, int op, size_t* offset_ints, size_t* count_ints);
int32_t tmac_hip_debug_chain_config(int force_waves_per_quad, unsigned spin_limit);
/* workgroups of chains built from now on (0 = one per CU): lets two chains run side by side on one device (tests/test_gpu_chain_ipc.py) */
int32_t tmac_hip_debug_chain_grid(int workgroups);
/* The stream-mode schedule as a pure function (no device is touched): n independent calls of items[i] lookup items each, `grid` row
 * ranges in `ncls` classes (a power of two <= 16, <= grid).  Call i is dealt to the aligned block of out_w[i] classes that starts at
 * class out_lo[i]; out_load[c] (may be NULL) = the items one range of class c walks over the launch.  `target` = the fewest items a
 * visit should give a range (TMAC_STREAM_VISIT_ITEMS), lpt != 0 = largest calls first (TMAC_STREAM_LPT). */
int32_t tmac_hip_debug_stream_schedule(const double* items, int n, int grid, int ncls, int target, int lpt, int32_t* out_lo, int32_t* out_w, double* out_load);

/* ---- multi-GPU exchange step ------------------------------------------------------------------
 * One process per GPU; weight ROWS are sharded over the ranks (tile-aligned; register a rank's tiles with
 * tmac_hip_register_weights: tiles are contiguous in the reference layout).  An M-tile needs only its own A / Scales
 * slice plus the WHOLE LUT (include/t-mac/tmac_gemm_wrapper.h:197-199), so the only exchange is an all-gather of what the
 * next LUT build needs whole: the activation block the shards produced (N x rows x 2 bytes), or int8 QLUT slices built from
 * a K slice (tmac_hip_workspace_ptrs gives the device pointers).  K is never split: integer sums stay bit-identical to
 * one GPU.  RCCL over xGMI, resolved with dlopen at the first call (single-GPU users need no RCCL).
 *   rank 0:     tmac_hip_comm_unique_id(id)  -> hand the TMAC_HIP_COMM_ID_BYTES to every rank (MPI, a file, a socket)
 *   every rank: hipSetDevice / tmac_hip_init(its GPU); tmac_hip_comm_init(&comm, id, rank, world)
 *   per step:   tmac_hip_comm_allgather(comm, my_part_dev, whole_dev, bytes_per_rank, stream)   (whole = world x bytes_per_rank)
 * Errors: tmac_hip_comm_last_error(). */
#define TMAC_HIP_COMM_ID_BYTES 128
typedef struct tmac_hip_comm tmac_hip_comm;
int32_t tmac_hip_comm_unique_id(void* id_out);
int32_t tmac_hip_comm_init(tmac_hip_comm** out, const void* id, int rank, int world);
int32_t tmac_hip_comm_allgather(tmac_hip_comm* comm, const void* send_dev, void* recv_dev, size_t bytes_per_rank, void* stream);
int32_t tmac_hip_comm_destroy(tmac_hip_comm* comm);
/* The same exchange step without RCCL: every rank owns a window in fine-grained device memory that all peers map through hipIpc*; a
 * small kernel publishes this rank's part and copies the peers' parts out of their windows (flags in the windows, no host in the
 * loop).  For nodes or tests where RCCL cannot serve -- several ranks on ONE device, for instance, which RCCL refuses.
 *   every rank: tmac_hip_comm_init_ipc(&comm, max_bytes_per_rank, rank, world);  tmac_hip_comm_export(comm, blob)
 *   all-gather the TMAC_HIP_COMM_BLOB_BYTES blobs over any transport (rank order);  tmac_hip_comm_connect(comm, blobs, world)
 *   per step:   tmac_hip_comm_allgather(comm, ...) as above (every rank issues the same sequence);  tmac_hip_comm_status after a
 *   synchronisation: 0, or a bit per rank whose part did not arrive in time.  HSA_ENABLE_IPC_MODE_LEGACY=0 where the driver has dmabuf IPC only. */
#define TMAC_HIP_COMM_BLOB_BYTES 128
int32_t tmac_hip_comm_init_ipc(tmac_hip_comm** out, size_t max_bytes_per_rank, int rank, int world);
int32_t tmac_hip_comm_export(const tmac_hip_comm* comm, void* blob_out);
int32_t tmac_hip_comm_connect(tmac_hip_comm* comm, const void* blobs_of_all_ranks, int world);
int32_t tmac_hip_comm_status(tmac_hip_comm* comm, uint32_t* error_word);
const char* tmac_hip_comm_last_error(void);

/* Raw device pointers of the workspace, for collectives (RCCL all-gather of the LUT over xGMI):
 *   qlut_dev  : kernel-layout half tables, nbytes_qlut per activation row
 *   lut_scales/lut_biases : fp32 [N][K/act_group_size] */
int32_t tmac_hip_workspace_ptrs(tmac_hip_workspace* ws, void** qlut_dev, size_t* nbytes_qlut_per_row,
                                void** lut_scales, void** lut_biases);

/* ---- (3) parity taps -------------------------------------------------------------------- */
/* QLUT in the reference layout int8 [N][K/4][16] + fp32 lut_scales/lut_biases [N][K/ags] -> host */
int32_t tmac_hip_workspace_read(tmac_hip_workspace* ws, int8_t* qlut_host, float* lut_scales_host,
                                float* lut_biases_host, int K, int N, int act_group_size, void* stream);
/* load a host-side reference-layout LUT into the workspace (what qgemm_lut_int8 does internally) */
int32_t tmac_hip_workspace_write(tmac_hip_workspace* ws, const int8_t* qlut_host, const float* lut_scales_host,
                                 const float* lut_biases_host, int K, int N, int act_group_size, void* stream);
/* Same kernel as tmac_hip_qgemm_dev with the integer tap enabled: PS_host int32 [N][M][K/ags] in the
 * reference's M-space (bit-plane) row order; for the unified-scale path [N][M] (K/ags == 1). */
int32_t tmac_hip_qgemm_partial_sums(const tmac_hip_weights* w, const tmac_hip_workspace* ws,
                                    int32_t* PS_host, int N, void* stream);
/* integer tap of the fused kernel (one matrix): PS_host as above, optional fp32 C_host [N][Mw], optional
 * lut_host [N][2][K/ags] = the LUT scales then biases the kernel built in LDS */
int32_t tmac_hip_qgemm_fused_partial_sums(const tmac_hip_weights* w, const void* B_dev, tmac_dtype_t act_dtype,
                                          int32_t* PS_host, float* C_host, float* lut_host, int N, void* stream);
/* Runs v_perm_b32 / v_mqsad_pk_u16_u8 / lookup4 on n quadruples of host words (in[4n] -> out[4n]); the
 * test-suite compares the result with the host models of tmac_amd/csrc/tmac_core.h. */
int32_t tmac_hip_selftest(const uint32_t* in_host, uint32_t* out_host, int n);
/* one wave of v_mfma_i32_16x16x64_i8: in[64][8] (A regs 0-3, B regs 4-7 per lane) -> out[64][4] (D regs) */
int32_t tmac_hip_selftest_mfma(const uint32_t* in_host, int32_t* out_host);
/* Select the GEMV kernel variant: 0 auto (fused layout where supported), 1/2 two-kernel tiled path
 * (mqsad / byte-add accumulate), 3 generic reference-layout kernel, 4 fused (v_mqsad accumulate),
 * 5 fused with the MFMA accumulate, 6 wave-per-row-quad kernel (QUAD layout, MFMA accumulate; what auto picks
 * for 1- to 4-bit weights), 7 the same with the v_mqsad accumulate.  Affects weights
 * registered AFTER the call (the variant fixes their device layout).  For A/B benchmarking and tests. */
int32_t tmac_hip_set_variant(int variant);
/* From n activation rows on the N > 1 entry points run an MFMA GEMM (k_gemm_planes, else k_gemm_onehot: the table gather written as
 * an int8 contraction, same bit-exact integer sums) instead of looping the GEMV kernel over the rows (qgemm.py:183-190); n = 0
 * disables it, any value other than the default 32 is taken literally.  At the default the library decides per launch: where
 * k_gemm_planes covers the configuration (1- to 4-bit weights with per-group scales and act groups of 64, 2-bit with a unified scale)
 * from the measured crossover on -- 7 to 16 rows depending on the matrices, tmac_dispatch.cpp gemm_pays; 12 rows through the split
 * entry points, whose LUT build does not know the matrix -- else from 32 rows (64 when the matrices of the call have fewer than
 * 128 x 64 output rows x bits / 2: an under-filled grid). */
int32_t tmac_hip_set_gemm_min_n(int n);
/* Fast aggregation (the reference's `-fa` build option, deploy/compile.py:167-174,223): the
 * looked-up bytes of an act group are folded by a tree of rounding-halving adds instead of being summed exactly
 * (SignedHalvingAdder, tbl.cc:86-141,201-256), the result rescaled by the group's table count and corrected by the
 * analytic bias (tbl.cc:301-318,474-477).  LOSSY; off by default as in every shipped reference configuration.
 *   0  exact sums (default)
 *   1  signed halving adds (vrhaddq_s8) -- the reference's ARM build, the one `-fa` is meant for
 *   2  the reference's AVX2 build (_mm256_avg_epu8 applied to the signed bytes): kept so that the implementation can
 *      be pinned bit for bit against reference code compiled on an x86 host; numerically meaningless
 * A build-time property in the reference, a registration-time property here: applies to weights registered AFTER the
 * call (they take the 16-table-segment layout and run the two-kernel path: preprocessor + qgemm).  Per-group-scale
 * weights with act_group_size 32 or 64 only, as in the reference (no fast aggregation on its int32 path). */
int32_t tmac_hip_set_fast_aggregation(int mode);
/* Measurement aid for bench.py: one launch that only reads `bytes` of device memory (non-temporal 16-byte loads) and
 * keeps nothing -- the cost of streaming a matrix's bytes with no LUT build and no lookups, under the same launch
 * mechanism as the GEMV it is compared with.  dev_sink: >= 4 KB of device scratch. */
int32_t tmac_hip_debug_stream_read(const void* dev_src, size_t bytes, void* dev_sink, void* stream);
/* A/B and profiling knobs (tools/, tests/): force the decode kernel's launch configuration (0, 0 = heuristic / tuned
 * table); s_memtime phase stamps [workgroups][2][8] of the next fused launches into a device buffer (NULL = off);
 * activation rows from which tmac_hip_preprocessor_dev builds the LUT pair-wise (k_preprocess_pairs; default 2). */
int32_t tmac_hip_debug_quad_config(int force_threads, int force_waves_per_quad);
int32_t tmac_hip_debug_stamps(unsigned long long* dev_buffer);
int32_t tmac_hip_debug_pairs_min_n(int n);
/* N > 1 kernel selection and parity taps.  0 (default): k_gemm_planes (bit-planes combined inside the matrix-core operand,
 * tmac_gemm2.hip) wherever it covers the configuration (1- to 4-bit weights with per-group scales and act_group_size 64; 2-bit
 * weights with a unified scale);
 * 1: always k_gemm_onehot (one matrix-core row per bit-plane row).  2 / 3: k_gemm_planes with its eight-wave (one workgroup per
 * CU) / four-wave (two per CU) workgroup form forced; 0 picks by the number of tiles of the launch (tmac_gemm2.hip, PForm).
 * tmac_hip_debug_gemm_comb_sums: int32 [N][Mw][K/64], the integers sum_p 2^p PS_p (PS_p as tmac_hip_qgemm_partial_sums
 * returns them per bit-plane) that k_gemm_planes feeds into the fp32 chain; the workspace must hold the LUT of a
 * tmac_hip_preprocessor_dev call with N >= 2 rows.  tmac_hip_debug_gemm_image_read: the LUT image that kernel streams,
 * in plain layouts: signed half tables int8 [N][K/4][8] (entry j of table t; entry 15 - j is its negation,
 * lut_ctor.cc:152-155), lut_scales, lut_biases and the sum of each act group's 128 half-table entries, fp32 [N][K/64]. */
int32_t tmac_hip_debug_gemm_kernel(int which);
/* profiling: workgroup 0 of the following k_gemm_planes launches writes s_memrealtime stamps [wave 8][step 64][8] into this
 * device buffer (NULL = off); tools/gemm2_stamps.py prints them.  The kernel honours it in profiling builds of the library only
 * (-DTMAC_G2_STAMPS=1; compiled out by default: the hook cost the 4-bit prefill line 1 %) -- otherwise the buffer stays untouched */
int32_t tmac_hip_debug_gemm_stamps(unsigned long long* dev_buffer);
int32_t tmac_hip_debug_gemm_comb_sums(const tmac_hip_weights* w, const tmac_hip_workspace* ws, int32_t* comb_host, int N, void* stream);
int32_t tmac_hip_debug_gemm_image_read(const tmac_hip_workspace* ws, int8_t* half_tables_host, float* lut_scales_host,
                                       float* lut_biases_host, float* entry_sums_host, int N, void* stream);
/* k_gemv_rows (tmac_rows.hip): N >= 2 activation rows below the GEMM crossover on QUAD-layout weights, 2 / 4 / 8 rows per pass over the
 * weights, the tables copied from the workspace's half-table image.  Taps (tmac_hip_qgemm_partial_sums, tmac_hip_qgemm_fused_partial_sums)
 * never run it.
 * tmac_hip_debug_rows_kernel: 0 (default) auto -- the kernel where it was measured faster than the routing without it (tmac_dispatch.cpp,
 *   rows_auto); 1 off -- that routing bit for bit; 2 forced -- every N >= 2 call the kernel covers takes it, whatever the GEMM thresholds
 *   say (tests, A/B).  tmac_hip_reset_state puts it back to 0.
 * tmac_hip_debug_rows_stats: k_gemv_rows launches since the library was loaded or reset (a host counter; a call makes one launch for its
 *   full row groups and one more when the last group has another capacity).
 * tmac_hip_debug_rows_plan: the row groups of an N-row call, a pure function (no device is touched).  r_fit: the largest of 8 / 4 / 2
 *   rows whose tables and LUT scales plus the kernel's fixed part fit 163840 bytes of LDS (lds_bytes: that footprint); ngroups =
 *   ceil(N / r_fit); cap[g] / live[g] (each NULL or at least ngroups entries): every group but the last holds r_fit rows, the last the
 *   remainder in the smallest capacity of 2 / 4 / 8 that takes it.  m_groups: -1 per-group scales, >= 1 unified (same footprint).
 *   TMAC_HIP_E_ARG when not even two rows fit.  Launches and the tap below group by this function alone.
 * tmac_hip_debug_rows_comb_sums: the integers k_gemv_rows feeds into its float part, for the LUT the workspace holds (N <= its rows), in
 *   the row grouping of an untapped call of that N: per-group scales int32 [N][Mw][K/64] = sum_p 2^p PS_p; unified scales
 *   int32 [N][Mw][bits], the exact per-plane totals. */
int32_t tmac_hip_debug_rows_kernel(int mode);
int32_t tmac_hip_debug_rows_stats(uint64_t* launches);
int32_t tmac_hip_debug_rows_plan(int K, int m_groups, int N, int32_t* r_fit, int32_t* ngroups, int32_t* cap, int32_t* live, size_t* lds_bytes);
int32_t tmac_hip_debug_rows_comb_sums(const tmac_hip_weights* w, const tmac_hip_workspace* ws, int32_t* comb_host, int N, void* stream);
/* host-pointer entry points: 1 (default) = tiles with contiguous weight / scale pointers are grouped into runs once they
 * have been seen, and a run's output is computed in one launch per LUT and handed out tile by tile; 0 = every tile call is
 * served on its own */
int32_t tmac_hip_debug_host_runs(int on);
/* test knob: 0 skips the synchronisation that orders tmac_hip_workspace_create's null-stream fills before the workspace's
 * first user on another stream -- the round-2 defect (all-zero LUT image), kept reproducible for tests/test_gpu_hostptr.py */
int32_t tmac_hip_debug_ws_fill_sync(int on);
/* Test hook of the deferred queue: the nth launch attempted by the following flushes (1-based; a flush issues its stream launches first,
 * then its single calls) returns TMAC_HIP_E_RUNTIME before anything is enqueued on the GPU -- a host-side `if`, the device is not touched.
 * One-shot; 0 clears it, tmac_hip_reset_state clears it. */
int32_t tmac_hip_debug_defer_fail(int nth);
/* Launch-configuration tuner of the fused decode kernel (the role autotvm's grid search over
 * (bm, kfactor, bn) plays for the reference's CPU kernels, python/t_mac/ops/base.py:84-127, qgemm.py:98-116).
 * tmac_hip_autotune_fused times every (threads per workgroup, waves per row quad) configuration of k_gemv_quad on the
 * given 1..4 registered matrices (the set that tmac_hip_qgemm_fused_dev will be called with, N = 1), on HBM-cold
 * rotating copies of the weights inside a replayed hipGraph, and records the fastest when it beats the built-in
 * heuristic by more than 4 %; later fused calls with the same (bits, K, rows, matrices, dtypes) use it.  Results do not
 * change (same kernel, same arithmetic).  best_ft = 0 on return means "the heuristic stands".  Allocates and frees its
 * own buffers (a few hundred MB); synchronous; not for use inside a stream capture.
 * tmac_hip_tune_save / tmac_hip_tune_load persist the table as text (return the number of entries, or < 0);
 * $TMAC_HIP_TUNE_FILE is loaded on the first fused call. */
int32_t tmac_hip_autotune_fused(const tmac_hip_weights* const* weights, int nmat, tmac_dtype_t act_dtype,
                                tmac_dtype_t out_dtype, int* best_ft, int* best_wpq, float* best_us, float* heuristic_us);
int32_t tmac_hip_tune_save(const char* path);
int32_t tmac_hip_tune_load(const char* path);
int32_t tmac_hip_tune_clear(void);

/* ---- (1) reference-named host-pointer entry points ---------------------------------------
 * Signatures identical to the generated deploy/tuned/<set>/kernels.h.  `m` is bm for qgemm_lut
 * (one M-tile; A/Scales/C are the tile pointers, tmac_gemm_wrapper.h:197-228) and Mw*bits for the
 * preprocessor.  Tile weights are uploaded on first use and cached by host pointer (llama.cpp
 * keeps weights mmap'd for the life of the model); tmac_hip_cache_clear() drops the cache.
 * Configuration (group_size, zero_point, act_group_size) comes from the loaded kcfg
 * (tmac_hip_load_kcfg / $TMAC_KCFG_FILE), exactly as the reference couples kernels to kcfg.ini.
 * What a tile call answers for (tests/test_gpu_hostptr_purity.py):
 *   - the LUT: always the bytes it is passed.  QLUT, LUT_Scales and LUT_Biases are compared in full with the LUT the cached
 *     result was computed from, on every tile call, whichever buffers they arrive in (about 6 us of a 42 us 4096 x 4096 GEMV
 *     of 64 tile calls, profiles/hostptr_purity.txt);
 *   - the weights and scales behind a cached pointer: taken as unchanged.  A replacement that changes every 16-byte window
 *     of a tile's weights or of its scales -- a model reloaded at the same addresses, two tiles exchanged, new scales -- is
 *     detected from a sample and the tile registered afresh; after any other in-place edit call tmac_hip_cache_clear(). */
int32_t qgemm_lut_int8(int m, int k, int n, int b, void* A, void* LUT, void* Scales, void* LUT_Scales,
                       void* LUT_Biases, void* C);
int32_t preprocessor_int8(int m, int k, int n, int b, void* B, void* LUT_Scales, void* LUT_Biases, void* QLUT);
int32_t tmac_hip_cache_clear(void);

/* shape-named kernels of the four checked-in sets (deploy/tuned/aarch64-<set>/kernels.h) */
#define TMAC_DECL_Q(bm, k, n, b) \
    int32_t qgemm_lut_t1_int8_m##bm##_k##k##_n##n##_b##b(void* A, void* LUT, void* Scales, void* LUT_Scales, void* LUT_Biases, void* C);
#define TMAC_DECL_P(m, k, n, b) \
    int32_t preprocessor_t1_int8_m##m##_k##k##_n##n##_b##b(void* B, void* LUT_Scales, void* LUT_Biases, void* QLUT);
/* llama-2-7b-2bit */
TMAC_DECL_Q(128, 4096, 1, 2) TMAC_DECL_Q(128, 11008, 1, 2)
TMAC_DECL_P(8192, 4096, 1, 2) TMAC_DECL_P(22016, 4096, 1, 2) TMAC_DECL_P(8192, 11008, 1, 2)
/* llama-2-7b-4bit */
TMAC_DECL_Q(1024, 4096, 1, 4) TMAC_DECL_Q(256, 4096, 1, 4) TMAC_DECL_Q(256, 11008, 1, 4)
TMAC_DECL_P(16384, 4096, 1, 4) TMAC_DECL_P(44032, 4096, 1, 4) TMAC_DECL_P(16384, 11008, 1, 4)
/* llama-3-8b-2bit */
TMAC_DECL_Q(256, 4096, 1, 2) TMAC_DECL_Q(512, 4096, 1, 2) TMAC_DECL_Q(128, 14336, 1, 2)
TMAC_DECL_P(28672, 4096, 1, 2) TMAC_DECL_P(8192, 14336, 1, 2) TMAC_DECL_P(2048, 4096, 1, 2)
/* hf-bitnet-3b */
TMAC_DECL_Q(128, 8640, 1, 2) TMAC_DECL_Q(128, 3200, 1, 2) TMAC_DECL_Q(320, 3200, 1, 2)
TMAC_DECL_P(6400, 8640, 1, 2) TMAC_DECL_P(17280, 3200, 1, 2) TMAC_DECL_P(6400, 3200, 1, 2)
#undef TMAC_DECL_Q
#undef TMAC_DECL_P

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* TMAC_HIP_H_ */
