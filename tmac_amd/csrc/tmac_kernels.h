// tmac_kernels.h — host-callable launchers of the gfx950 kernels (implemented in tmac_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tmac_layout.h"
#include "tmac_launch_plan.h"      // what the fused kernels support, and how a launch is planned (plain C++)

namespace tmac {

enum Dtype { F32 = 0, F16 = 1 };

// GEMV kernel variants (A/B-able at run time through tmac_hip_set_variant)
enum Variant {
    V_AUTO = 0,      // k_gemv_quad (V_QUAD) where it supports the configuration, else the row-block fused kernel, else 1
    V_LO_MQSAD = 1,  // two-kernel path: k_preprocess + tiled k_gemv_lo, v_mqsad_pk_u16_u8 accumulate
    V_LO_SDWA = 2,   // same, byte-select adds
    V_REF_LAYOUT = 3,// generic kernel on the reference blobs (reference float order)
    V_FUSED = 4,     // row-block fused kernel k_gemv_fused (ts = 8 layout): LUT in LDS, v_mqsad accumulate
    V_FUSED_MFMA = 5,// same kernel with the matrix-pipe (v_mfma_i32_16x16x64_i8) accumulate
    V_QUAD = 6,      // wave-owns-row-quad fused kernel k_gemv_quad (QUAD layout), MFMA accumulate
    V_QUAD_MQSAD = 7 // same with the v_mqsad_pk_u16_u8 accumulate (512-thread workgroups)
};

struct FusedMat {
    const uint4* W;   // ts = 8 device layout
    const void* SC;   // device layout scales (or [m_groups] unified scales)
    void* C;          // [N][Mw]
    int Mw;
    int nb_end;       // cumulative number of 16-row blocks up to and including this matrix
};

struct FusedArgs {
    FusedMat m[4];
    int nmat;
    Shape s;                 // K, bits, gs, ags, zero_point, m_groups, ts = 8 (Mw unused)
    const void* B;           // activations [N][K]                       (LUT built in-kernel)
    int act_f16;
    const void* qlut_lds;    // uint4 [N][qlut_lds_u4(K)]                (LUT prebuilt by k_preprocess)
    const float* lut_scales; // fp32 [N][K/ags]
    const float* lut_biases;
    int sc_f16, out_f16;
    int32_t* dump;           // optional integer tap (nmat == 1)
    unsigned long long* stamps; // optional s_memtime phase stamps [blocks][8] (debug/profiling)
    float* lut_tap;          // optional: block 0 writes [N][2][G] LUT scales | biases it built (parity tap)
    int acc_mfma;            // 1: v_mfma_i32_16x16x64_i8 accumulate, 0: v_mqsad_pk_u16_u8 (default: measured faster, profiles/)
    int nu, nsb, tstride, G, nsg, gs_shift;   // filled by the launchers (fused_precompute, tmac_launch_plan.h: host-side divides)
};

// k_gemv_quad's XF instantiations (tmac_hip_qgemm_fused_xf_dev): the N = 1 call plus a vector transform of its activations, applied
// between the activation loads and the table build.  An argument block of its own: the plain instantiations keep theirs.
struct FusedXfArgs : FusedArgs {
    int xf_kind;             // TMAC_XF_NORM (1) | TMAC_XF_GLU (2) | TMAC_XF_GLU_NORM (4); GLU, GLU_NORM: | the gate << 8 (0 silu, 1 relu^2, 2 tanh-GELU:
                             // tmac_quad_core.h XF_GATE_*) -- tmac_hip_xform::kind as it comes.  (No field of its own: the block keeps its size,
                             // and the instantiations that never look at the gate their code)
    const void* in2;         // GLU, GLU_NORM: second vector [K], dtype of B
    const float* residual;   // NORM: fp32 [K] or null
    const float* gamma;      // NORM: fp32 [K] or null (add only); GLU_NORM: fp32 [K], required
    float* residual_out;     // NORM: fp32 [K] or null; pair p is stored by workgroup p mod gridDim.x
    float eps;
};

// k_gemv_quad's gather instantiations (a fused N = 1 call on act-order handles): the LUT build loads x[perm[k']] for position k'.  An argument
// block of its own: the plain instantiations keep theirs.
struct FusedPermArgs : FusedArgs {
    const int32_t* perm;     // int32 [K], every value < K, 16-byte aligned (tmac_hip_kperm)
};

// k_gemv_quad's bias instantiations (BI: handles registered with a bias, tmac_hip_weights_set_bias_dev): y = W x + b, the add in front of
// the output's one store.  bias[i]: the handle's own fp32 copy for matrix i ([Mw] padded with zeros to a multiple of 64 elements,
// 256-byte aligned), or null -- the matrix has none and stores what the plain call stores.  Argument blocks of their own, plain and
// transformed: the other instantiations keep theirs.
struct FusedBiasArgs : FusedArgs {
    const float* bias[4];
};
struct FusedXfBiasArgs : FusedXfArgs {
    const float* bias[4];
};

// The same transforms for N > 1 activation rows (tmac_hip_qgemm_fused_xf_rows_dev): the argument block of k_xf_rows (the row pass: residual_out
// and 1 / rms per row) and of the XF instantiations of the three N > 1 LUT builders (k_lut_image, k_preprocess_pairs, k_preprocess_pairs_row),
// which replace their activation load by xf_rows_x8 (tmac_quad_core.h).  Row n of every [N][K] operand is read for row n of the activations.
struct XfRowsArgs {
    int kind;                // TMAC_XF_NORM (1) | TMAC_XF_GLU (2) | TMAC_XF_GLU_NORM (4)
    const void* in2;         // GLU, GLU_NORM: [N][K], dtype of B
    const float* residual;   // NORM: fp32 [N][K] or null
    const float* gamma;      // NORM: fp32 [K] (shared by the rows) or null (add only); GLU_NORM: fp32 [K], required
    const float* r;          // NORM with gamma, GLU_NORM: fp32 [N], 1 / rms of row n, written by k_xf_rows
    float* residual_out;     // NORM: fp32 [N][K] or null; written by k_xf_rows alone
    float eps;
};
// ... with the gate of a GLU / GLU_NORM as a run-time choice: what the host passes down, and the argument block of the kernels' instantiations
// for relu^2 and GELU (xf_rows_g8 reads `gate` where the block has one).  A call with silu runs the instantiations on the plain block above:
// the code and the registers they had before the selector existed (profiles/r14_gate_resources.txt).
struct XfRowsGateArgs : XfRowsArgs {
    int gate;                // 0 silu | 1 relu^2 | 2 tanh-GELU (tmac_quad_core.h XF_GATE_*)
};
// the launchers' selector of the two: f(the block the call's instantiation takes)
template <class F>
inline hipError_t sel_xf_block(const XfRowsGateArgs& xf, F&& f) { return xf.gate == 0 ? f(static_cast<const XfRowsArgs&>(xf)) : f(xf); }

// one-hot MFMA GEMM for N > 1 activation rows (tmac_gemm.hip); weights in the QUAD layout; up to 4 matrices that share
// K, the quantisation config and the LUT in one launch
struct GemmMat {
    const void* W;            // QUAD layout weights
    const void* SC;           // QUAD layout scales
    void* C;                  // [N][Mw]
    int Mw;
    int wg_end;               // cumulative workgroup count along x (filled by the launcher)
};
struct GemmArgs {
    Shape s;                  // K, bits, gs, ags, zero_point (Mw unused)
    GemmMat m[4];
    int nmat;
    int sc_f16, out_f16;
    const void* qlut_lds;     // uint4 [N][4][tstride]: half tables, unit-major image written by k_preprocess
    int tstride;
    const float* lut_scales;  // fp32 [N][K/ags]
    const float* lut_biases;
    int32_t* dump;            // optional integer tap [N][M][K/ags] (nmat == 1)
    int N;
};

// plane-combined one-hot GEMM (tmac_gemm2.hip): the LUT comes as the image k_lut_image writes
struct Gemm2Args {
    Shape s;                  // K, bits, gs, ags = 64, zero_point (Mw unused)
    GemmMat m[4];
    int nmat;
    int sc_f16, out_f16;
    const uint4* bimg;        // per-group scales (k_lut_image): uint4 [K/64][Npad/64][8][64], the chunk of (act group, 64 rows) in one piece | unified
                              // scales (k_preprocess_pairs_row): uint4 [K/32 units][4 pairs][Npad]: signed half tables of tables 2P, 2P+1 of the unit
    const float* colv;        // per-group: float4 [K/64][Npad] = lut_scales / 2 | lut_biases / 2 | entry sum | lut_biases;  unified: fp32 [3][Npad]
    int Npad, N;
    int32_t* dump;            // optional tap [N][Mw][K/64]: sum_p 2^p PS_p (nmat == 1)
    int gx, gy;               // filled by the launcher: row blocks (64 rows, all matrices) and token blocks (64 rows of activations)
    int apg_shift;            // filled by the launcher: log2(act groups per weight group)
    unsigned long long* stamps; // optional s_memrealtime stamps of workgroup 0: [wave 8][step 64][8] (profiling; tools/gemm2_stamps.py)
    int form;                 // 0: by the number of tiles | 1: eight-wave workgroups, one per CU | 2: four-wave workgroups, two per CU
};
// k_gemm_planes' bias instantiations (per-group scales): bias[i] as in FusedBiasArgs, added to the four outputs of a store
struct Gemm2BiasArgs : Gemm2Args {
    const float* bias[4];
};

struct GemvArgs {
    Shape s;
    const void* W;        // device layout weights (uint4)        | reference blob for V_REF_LAYOUT
    const void* SC;       // device layout scales (sc_dtype)      | reference blob (float_type = sc_dtype)
    Dtype sc_dtype;
    const void* qlut_dev; // uint4 [N][qlut_dev_u4]
    const int8_t* qlut_ref; // int8 [N][K/4][16] (V_REF_LAYOUT only)
    const float* lut_scales;
    const float* lut_biases;
    void* C;              // [N][Mw]
    Dtype out_dtype;
    int32_t* ps_dump;     // optional int32 tap (device)
    int N;
    int fa_mode;          // 0 exact sums | 1, 2: fast aggregation (a9; see SegAcc<BITS, 2> in tmac_core.h)
};

hipError_t launch_selftest(const uint32_t* in, uint32_t* out, int n, hipStream_t st);
hipError_t launch_selftest_mfma(const uint32_t* in, int32_t* out, hipStream_t st);
hipError_t launch_selftest_permlane(const uint32_t* in, uint32_t* out, hipStream_t st);
hipError_t launch_retile_weights(const uint8_t* A_ref, void* Wd, const Shape& s, hipStream_t st);
hipError_t launch_retile_scales(const void* S_ref, Dtype in_dt, void* Sd, Dtype out_dt, const Shape& s, hipStream_t st);
// device-side packing (tmac_pack.hip): GPTQ tensors (bits 1, 2, 4; per-group scales) or plain codes (bits 1-4) -> the reference blob halves
// A_out (ref_weight_bytes) and S_out (ref_scale_elems values of out_dt).  qzeros / zeros NULL = no zero points.  perm (device, int32 [K],
// every value < K, 16-byte aligned; NULL = none): act-order -- the blob of the matrix whose column k' is source column perm[k'].
hipError_t launch_pack_gptq(const void* qweight, const void* scales, const void* qzeros, Dtype scales_dt, int gptq_v2, void* A_out, void* S_out,
                            Dtype out_dt, const Shape& s, hipStream_t st, const int32_t* perm = nullptr);
hipError_t launch_pack_codes(const void* codes, const void* scales, const void* zeros, Dtype sz_dt, void* A_out, void* S_out, Dtype out_dt,
                             const Shape& s, hipStream_t st, const int32_t* perm = nullptr);
// AutoAWQ tensors (WQLinear_GEMM: qweight int32 [K][Mw / 8], scales [K / gs][Mw], qzeros int32 [K / gs][Mw / 8] or NULL = no zero points;
// the format: tmac_pack.h), bits = 4, per-group scales, Mw a multiple of 8 -> the same two halves.
hipError_t launch_pack_awq(const void* qweight, const void* scales, const void* qzeros, Dtype scales_dt, void* A_out, void* S_out, Dtype out_dt,
                           const Shape& s, hipStream_t st);
// BitNet master weights W [Mw][K] (src: tmac_src_dtype_t; 16-byte aligned, K a multiple of 4, Mw of m_groups).  launch_absmean: the fp32
// scale of each of the m_groups row blocks, fmaxf(mean |w|, eps), through `partials` (absmean_partial_count doubles of scratch).
// launch_pack_dense: bits = 2, unified scales -- the levels of the absmean rule under `scales` (fp32 [m_groups], all > 0) straight into
// A_out, and the scales into S_out as out_dt.
size_t absmean_partial_count(int Mw, int K, int m_groups);
hipError_t launch_absmean(const void* W, int src, int Mw, int K, int m_groups, float eps, double* partials, float* scales_out, hipStream_t st);
hipError_t launch_pack_dense(const void* W, int src, const float* scales, void* A_out, void* S_out, Dtype out_dt, const Shape& s, hipStream_t st);
// Dense master weights W [Mw][K] -> W1 - W4 with per-group scales, round to nearest (the rule: tmac_pack.h; gs a multiple of 4 that divides
// K).  launch_rtn_params: fp32 [Mw][K / gs] each -- the scale, the zero code zq and (zeros != NULL) T-MAC's zero of every (row, group);
// invalid (device int32, NULL = not counted): the invalid groups are ADDED to it, at most one atomicAdd per workgroup; the caller zeroes it.
// launch_pack_rtn: per-group scales only -- the codes under (scales, zq) straight into A_out, scales and zeros (NULL exactly without zero
// points) into S_out as out_dt.
hipError_t launch_rtn_params(const void* W, int src, int Mw, int K, int bits, int gs, int zero_point, int scale_f16, float* scales, float* zq, float* zeros,
                             int32_t* invalid, hipStream_t st);
hipError_t launch_pack_rtn(const void* W, int src, const float* scales, const float* zq, const float* zeros, void* A_out, void* S_out, Dtype out_dt,
                           const Shape& s, hipStream_t st);
// BitNet packed ternary checkpoints: packed uint8 [Mw / 4][K] (four weight rows per byte: tmac_pack.h; 16-byte aligned), bits = 2, unified
// scales -- the levels straight into A_out, `scales` (fp32 [m_groups]) into S_out as out_dt.  invalid (device int32, NULL = not counted):
// the fields of value 3 are ADDED to it, at most one atomicAdd per workgroup; the caller zeroes it.  The read-once kernel
// (k_pack_ternary_weights_x4) where pack_ternary_reads_once(s), i.e. (Mw / 4) % 16 == 0, unless `general` forces k_pack_ternary_weights.
bool pack_ternary_reads_once(const Shape& s);
hipError_t launch_pack_ternary(const void* packed, const float* scales, void* A_out, void* S_out, Dtype out_dt, const Shape& s, int32_t* invalid,
                               bool general, hipStream_t st);
hipError_t launch_preprocess(const void* B, Dtype act_dt, int8_t* qlut_ref, void* qlut_dev, void* qlut_lds, float* lut_scales,
                             float* lut_biases, int K, int N, int ags, size_t qdev_u4_per_row, hipStream_t st);
// all-gather over IPC-mapped windows (tmac_comm.cpp, transport "ipc"): workgroup p of `world` handles rank p's part
struct IpcGatherArgs {
    const unsigned char* send;     // this rank's part
    unsigned char* recv;           // world x bytes
    size_t bytes;                  // per rank
    unsigned char* win[8];         // every rank's window (own + the peers' as mapped into this process): two halves of win_half bytes
    unsigned* flag[8];             // every rank's two flag words (generation of the all-gather whose part the half holds)
    size_t win_half;
    int rank, world;
    unsigned gen;                  // 1, 2, ...: half = gen & 1
    unsigned spin_limit;
    unsigned* err;                 // set when a peer's part did not arrive
};
hipError_t launch_ipc_allgather(const IpcGatherArgs& a, hipStream_t st);
hipError_t launch_qlut_ref_to_dev(const int8_t* qlut_ref, void* qlut_dev, void* qlut_lds, int K, int N, size_t qdev_u4_per_row, hipStream_t st);
// pair-wise LUT build (tmac_prefill_lut.hip; ags = 64): the half-table image + LUT scales/biases, and -- when qlut_ref / qlut_dev are
// given (both or neither) -- the other two layouts of the workspace as well
hipError_t launch_preprocess_pairs(const void* B, int act_f16, void* qlut_lds, float* lut_scales, float* lut_biases, int K, int N,
                                   int8_t* qlut_ref, void* qlut_dev, size_t qdev_u4_per_row, hipStream_t st, const XfRowsGateArgs* xf = nullptr,
                                   const int32_t* perm = nullptr);
// (perm, here and at launch_lut_image: the gather instantiation of an act-order permutation -- x = row n read through perm (device, int32 [K],
// every value < K, 16-byte aligned) instead of the row itself; never together with xf; with qlut_ref / qlut_dev it writes every layout)
// the same for act_group_size = K (one act group per activation row; K <= 12288)
// bimg / colv (both or neither; Npad = row stride of the image): also the LUT image k_gemm_planes_us streams (tmac_gemm2.hip)
hipError_t launch_preprocess_pairs_row(const void* B, int act_f16, void* qlut_lds, float* lut_scales, float* lut_biases, int K, int N,
                                       int8_t* qlut_ref, void* qlut_dev, size_t qdev_u4_per_row, void* bimg, float* colv, int Npad, hipStream_t st,
                                       const XfRowsGateArgs* xf = nullptr);
// xf (all three builders, and launch_lut_image below): the XF instantiation -- x = the transform of row n instead of the row itself; the
// half-table image / LUT image alone (qlut_ref and qlut_dev must be null).  launch_xf_rows: the row pass in front of it (NORM with gamma or
// residual_out; r_out: fp32 [N] or null); launch_xf_rows_tap: the fp32 x [N][K] the builders consume (tmac_hip_debug_xf_rows).
hipError_t launch_xf_rows(const XfRowsGateArgs& xf, const void* B, int act_f16, float* r_out, int K, int N, hipStream_t st);
hipError_t launch_xf_rows_tap(const XfRowsGateArgs& xf, const void* B, int act_f16, float* x_out, int K, int N, hipStream_t st);
hipError_t launch_stream_read(const void* src, size_t bytes, void* sink, hipStream_t st);
// host-pointer route (tmac_kernels.hip): results into pinned host memory by the GPU's own stores, then a flag the host spins on
hipError_t launch_host_copy3_flag(const void* q, size_t nq, const void* ls, const void* lb, size_t ns, void* dst_pinned, uint32_t* flag,
                                  uint32_t val, hipStream_t st);
hipError_t launch_host_flag(uint32_t* flag, uint32_t val, hipStream_t st);   // measurement aid, see tmac_kernels.hip
bool gemm_onehot_supported(const Shape& s);
hipError_t launch_gemm_onehot(const GemmArgs& a, hipStream_t st);
bool gemm_planes_supported(const Shape& s);
hipError_t launch_lut_image(const void* B, int act_f16, void* bimg, float* colv, int K, int N, int Npad, hipStream_t st, const XfRowsGateArgs* xf = nullptr,
                            const int32_t* perm = nullptr);
hipError_t launch_gemm_planes(const Gemm2Args& a, hipStream_t st);
// ... with a bias on at least one matrix (per-group scales, no tap: anything else is hipErrorInvalidValue)
hipError_t launch_gemm_planes(const Gemm2BiasArgs& a, hipStream_t st);
// a handle's own copy of its bias (tmac_pack.hip): bias [Mw] of dtype src (tmac_src_dtype_t) -> fp32 out [Mpad], elements Mw .. Mpad - 1 zero
hipError_t launch_bias_copy(const void* bias, int src, float* out, int Mw, int Mpad, hipStream_t st);
// fused kernel (tmac_fused.hip)
size_t qlut_lds_u4(int K);   // uint4 per activation row of the LDS-image LUT
hipError_t launch_gemv_fused(const FusedArgs& a, int N, bool build_lut, hipStream_t st);
// quad kernel (tmac_quad.hip, one translation unit per width and scale dtype; the entry points: tmac_launch.cpp): a.m[i].nb_end =
// cumulative ROW QUAD counts; ft / wpq: 0 = heuristic.  One signature for the three argument blocks.  strict: the configuration was forced
// by the caller and must be covered as it is (hipErrorInvalidValue otherwise) -- else it falls back to the nearest covered one; the plain
// block ignores it: every configuration exists for it.
hipError_t launch_gemv_quad(const FusedArgs& a, int N, bool build_lut, int ft, int wpq, bool strict, hipStream_t st);
// The same kernel with a vector transform in front of its table build (N = 1, LUT built in-kernel, MFMA accumulate: anything else is
// hipErrorInvalidValue).  The XF instantiations cover a subset of the launch configurations (quad_xf_covered, tmac_launch_plan.h).
hipError_t launch_gemv_quad(const FusedXfArgs& a, int N, bool build_lut, int ft, int wpq, bool strict, hipStream_t st);
// ... and with the gather of an act-order permutation in its activation loads (N = 1, LUT built in-kernel, MFMA accumulate, per-group
// scales): the same covered configurations, the same fall-back.
hipError_t launch_gemv_quad(const FusedPermArgs& a, int N, bool build_lut, int ft, int wpq, bool strict, hipStream_t st);
// ... and with a bias added at the store (MFMA accumulate, per-group scales, no tap; any N): the LUT built in-kernel in the covered
// configurations with the same fall-back, or copied from the workspace's image (512-thread workgroups: both are covered).  The transformed
// form: N = 1, NORM and the silu GLU.
hipError_t launch_gemv_quad(const FusedBiasArgs& a, int N, bool build_lut, int ft, int wpq, bool strict, hipStream_t st);
hipError_t launch_gemv_quad(const FusedXfBiasArgs& a, int N, bool build_lut, int ft, int wpq, bool strict, hipStream_t st);
// the launcher of one translation unit of tmac_quad.hip (defined and instantiated there for its BITS, SCF16 and both argument blocks): the
// instantiation the plan names; a: precomputed (fused_precompute).  (Also for FusedPermArgs.)
template <int BITS, bool SCF16, class Args>
hipError_t launch_gemv_quad_unit(const Args& a, const QuadPlan& p, int N, hipStream_t st);
// rows kernel (tmac_rows.hip): 2-8 activation rows per weight pass on QUAD-layout weights, tables copied from the half-table image
struct RowsArgs {
    FusedMat m[4];           // nb_end = cumulative ROW QUAD counts (fill_fused_args)
    int nmat;
    Shape s;                 // K, bits, gs, ags, zero_point, m_groups (Mw unused)
    const void* qlut_lds;    // uint4 [N][qlut_lds_u4(K)]: the half-table image of the pair builds / k_preprocess
    const float* lut_scales; // fp32 [N][K/ags]
    const float* lut_biases;
    int sc_f16, out_f16;
    int32_t* tap;            // optional (nmat == 1): int32 [N][Mw][K/64] = sum_p 2^p PS_p | unified scales: [N][Mw][bits] plane totals
    int N;
    // filled by the launcher
    int nu, nst, tstride, G, nsg, gs_shift;   // tstride: of the IMAGE (the LDS copy uses nst * 64 + 1)
    int wpq;                 // waves per row quad (1, 2, 4): fixed by the shape alone
    int n_base, rows_per_group;   // rows of workgroup row y: n_base + y * rows_per_group ..., min(R, N - first) of them live
};
// (the row groups of N rows, the waves per quad and the launches: rows_launch_plan, tmac_launch_plan.h)
// *launches (optional) grows by the number of k_gemv_rows launches made (one for the full groups, one for a last group of another capacity)
hipError_t launch_gemv_rows(const RowsArgs& a, hipStream_t st, int* launches);
// the launcher of one translation unit of tmac_rows.hip (defined and instantiated there for its BITS): one planned launch
template <int BITS>
hipError_t launch_gemv_rows_unit(const RowsArgs& a, const RowsLaunch& l, hipStream_t st);
// returns hipErrorInvalidValue when the variant does not cover the configuration
hipError_t launch_gemv(const GemvArgs& a, Variant v, hipStream_t st);
bool gemv_lo_supported(const Shape& s);

}  // namespace tmac
