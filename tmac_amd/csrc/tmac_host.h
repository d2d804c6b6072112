// tmac_host.h — internals shared by the host-side translation units of libtmac_hip.so (nothing here is exported; the
// export list is include/tmac_hip.h).
//
//   tmac_runtime.cpp     error text, device binding, the knob block, lifecycle, self-tests, tmac_hip_reset_state
//   tmac_kcfg.cpp        the kcfg.ini table and its lookups
//   tmac_weights.cpp     weight registration (reference layout -> device layout)
//   tmac_bias.cpp        the bias of a handle (y = W x + b): tmac_hip_weights_set_bias_dev, the handle's own fp32 copy
//   tmac_kperm.cpp       the K permutation of act-order matrices from g_idx (tmac_kperm.h: no HIP, builds with plain g++); its C-ABI: tmac_pack_host.cpp
//   tmac_pack_host.cpp   device-side packing: GPTQ tensors / plain codes -> reference blob (tmac_pack.hip) -> register_impl
//   tmac_workspace.cpp   LUT workspace: the preprocessor entry points, lut_build (the one caller of the LUT builders; what a workspace holds and
//                        which launches put it there: tmac_lut_held.h, no HIP, plain g++), the per-stream workspaces of the fused entry point
//   tmac_xform.cpp       the field rules of tmac_hip_xform: one resolver for every transform site (tmac_xform.h: no HIP, builds with plain g++)
//   tmac_launch_plan.cpp launch planning of k_gemv_quad / k_gemv_rows and what the fused kernels support: pure functions that fill a plan or refuse
//                        (tmac_launch_plan.h: also the instantiation policy of every kernel family as constexpr predicates; no HIP, plain g++)
//   tmac_launch.cpp      launch_gemv_quad (one overload per argument block) / launch_gemv_rows / launch_decode_chain / launch_gemv_stream: plan,
//                        pick the translation unit of the call's width or form; the unit selects the instantiation (tmac_select.h) and launches
//   tmac_dispatch.cpp    qgemm_lut dispatch (a call is planned -- enum Route -- then launched); the fused entry point: its doors, the named
//                        checks they share, plan_call, the one k_gemv_quad launch site (a fused call is one value: FusedCall, below); parity taps
//   tmac_tuner.cpp       launch-configuration tuner of the decode kernel
//   tmac_chain_host.cpp  recording and building the persistent decode chain (chain_build and its stages, the stream schedule)
//   tmac_chain_launch.cpp  launching a built chain, IPC export / connect, status, info, taps, stamps
//   tmac_defer.cpp       the deferred queue (tmac_hip_defer / tmac_hip_flush)
//                        (the three share tmac_chain_host.h: struct tmac_hip_chain, the noted calls, chain_build)
//   tmac_hostptr.cpp     the reference-named host-pointer entry points (struct HostRoute)
//   tmac_comm.cpp        multi-GPU exchange step (RCCL)
#pragma once
#include <hip/hip_runtime.h>

#include <array>
#include <chrono>
#include <climits>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/tmac_hip.h"
#include "tmac_chain.h"
#include "tmac_kernels.h"
#include "tmac_kperm.h"
#include "tmac_lut_held.h"
#include "tmac_xform.h"

// ---- the C-ABI's opaque objects ---------------------------------------------------------------
// The K permutation of act-order matrices (tmac_kperm.h): host copy, hash, and the device copy the gathers read (int32 [K], hipMalloc:
// 256-byte aligned).  Shared: the caller's object and every handle registered through it hold one reference each.
struct KPermData {
    tmac_host::KPermHost h;
    int32_t* dev = nullptr;
    ~KPermData() { if (dev) (void)hipFree(dev); }
};
struct tmac_hip_kperm { std::shared_ptr<KPermData> d; };

struct tmac_hip_weights {
    tmac::Shape s;
    void* W = nullptr;      // device layout weights
    void* SC = nullptr;     // device layout scales
    tmac::Dtype sc_dtype = tmac::F32;
    void* A_ref = nullptr;  // reference blobs kept on the device only when the generic kernel needs them
    void* S_ref = nullptr;
    tmac::Dtype ref_dtype = tmac::F32;
    bool tiled_ok = false;  // W / SC hold the device layout s names (layout_of) and its tiled kernel covers the configuration; else only the reference blobs serve
    int fa = 0;             // fast-aggregation mode these weights were registered under (0 = exact)
    size_t w_bytes = 0, sc_bytes = 0;
    std::shared_ptr<KPermData> kperm;   // act-order: the matrix is W[:, perm] and every LUT build gathers x[perm]; null = none
    float* bias = nullptr;  // y = W x + b (tmac_hip_weights_set_bias_dev): the handle's own fp32 copy, [Mw] padded with zeros to a multiple of 64 elements; null = none
};

struct tmac_hip_workspace {
    int maxK = 0, maxN = 0;
    int8_t* qlut_ref = nullptr;  // int8 [maxN][maxK/4][16]
    void* qlut_dev = nullptr;    // uint4 [maxN][qdev_u4(maxK)]   (ts = 16 layout)
    void* qlut_lds = nullptr;    // uint4 [maxN][qlut_lds_u4(K)]  (LDS image for the fused-layout kernel)
    float* lut_scales = nullptr; // fp32 [maxN][maxK/32]
    float* lut_biases = nullptr;
    int32_t* dump = nullptr;     // lazily sized parity tap
    size_t dump_elems = 0;
    tmac_host::LutHeld held;     // what the buffers above and the LUT image below hold (tmac_lut_held.h): changed by lut_build and tmac_hip_workspace_write alone
    // the LUT as k_gemm_planes streams it (tmac_gemm2.hip): built next to the layouts above when N > 1
    void* gimg = nullptr;        // 2 maxK gNpad bytes: the LUT image of the plane-combined GEMM (layouts: Gemm2Args, tmac_kernels.h)
    float* gcol = nullptr;       // 4 (maxK / 64) gNpad floats: its column values
    int gNpad = 0;               // its row stride: maxN rounded up to 64
    float* xf_r = nullptr;       // fp32 [maxN]: 1 / rms per activation row of a transformed N > 1 call (k_xf_rows -> the XF LUT builders)
    // can k_gemm_planes address the LUT image of K at this row stride (below 2 GB)?
    bool image_fits(int K) const { return gimg && (size_t)2 * K * gNpad < ((size_t)1 << 31); }
};

namespace tmac_host {
using namespace tmac;

// ---- errors -----------------------------------------------------------------------------------
// fail(code, fmt, ...) sets the thread's message and returns code: declared in tmac_xform.h, defined in tmac_runtime.cpp

// device scratch of the test taps and self-tests: freed on every return path
struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes); }
    template <class T> T* as() const { return static_cast<T*>(p); }
};

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return ::tmac_host::fail(TMAC_HIP_E_RUNTIME, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                                     __FILE__, __LINE__);                                          \
    } while (0)

// ---- process-wide state -----------------------------------------------------------------------
// Every tmac_hip_set_* / tmac_hip_debug_* setting lives in this one block; tmac_hip_reset_state() assigns a fresh one.
struct Knobs {
    int variant = V_AUTO;          // tmac_hip_set_variant
    int gemm_min_n = 32;           // tmac_hip_set_gemm_min_n: measured crossover on MI355X (llama-2-7B W2 shapes): GEMV loop ~1.7 us per row, GEMM 40-60 us up to 64 rows
    int gemm_kernel = 0;           // N > 1 kernel: 0 = k_gemm_planes where it covers the configuration, 1 = k_gemm_onehot, 2 / 3 = k_gemm_planes forced to eight- / four-wave workgroups (tmac_hip_debug_gemm_kernel)
    int pairs_min_n = 2;           // tmac_hip_preprocessor_dev: rows from which the pair-wise LUT build is used (tmac_hip_debug_pairs_min_n)
    int fa_mode = 0;               // fast aggregation for weights registered from now on (tmac_hip_set_fast_aggregation)
    int force_ft = 0, force_wpq = 0;   // A/B knobs of the quad kernel (0 = heuristic)
    int host_runs = 1;             // host-pointer layer: group contiguous tiles into runs (tmac_hip_debug_host_runs)
    int ws_fill_sync = 1;          // test knob (tmac_hip_debug_ws_fill_sync): 0 re-opens the round-2 race between the workspace fills and its first user
    int chain_wpq = 0;             // waves per row quad for every op of chains built from now on (0 = per-op choice)
    unsigned chain_spin_limit = 1u << 18;   // polls of one hand-off before a wave gives up (~0.4 s)
    int defer_fail = 0;            // test hook (tmac_hip_debug_defer_fail): the n-th launch attempted by the deferred queue's flushes fails on the host side; one-shot
    int rows_kernel = 0;           // k_gemv_rows: 0 = where measured faster, 1 = never (the routing without it), 2 = wherever it covers the call (tmac_hip_debug_rows_kernel)
    uint64_t rows_launches = 0;    // k_gemv_rows launches since load or reset (tmac_hip_debug_rows_stats): a counter, reset with the settings
    uint64_t route_launches[8] = {};   // launches per planned route, indexed by enum Route of tmac_dispatch.cpp (tmac_hip_debug_route_stats): counters, reset with the settings
    int pack_ternary_kernel = 0;   // packed ternary weights: 0 = the read-once kernel where it applies, 1 = k_pack_ternary_weights (the general form) everywhere (tmac_hip_debug_pack_ternary_kernel)
    int chain_grid = 0;            // workgroups of chains built from now on (0 = one per CU; tests run two chains side by side on one device)
    unsigned long long* stamps = nullptr;        // phase stamps of the next fused launches (tmac_hip_debug_stamps)
    int32_t* stamp_dump = nullptr;               // scratch the stamp instantiation stores its tap into (allocated once, survives resets)
    unsigned long long* gemm_stamps = nullptr;   // k_gemm_planes step stamps (tmac_hip_debug_gemm_stamps)
};
extern Knobs g_knobs;
extern std::mutex g_mu;       // kcfg table, the fused entry point's workspace map, the slow path of the host-pointer layer
extern int g_device;

// tmac_hip_init selects the device for the calling thread only (hipSetDevice is per thread); entry points reached from other
// threads -- llama.cpp calls qgemm_lut_int8 from every worker -- bind to the same device on their first call.
void bind_thread_device();
int32_t ensure_device();

constexpr int PLANES_MIN_N = 12;   // default GEMM threshold where k_gemm_planes covers the configuration (tmac_dispatch.cpp)
// Fewest activation rows that go to a GEMM instead of the row loop: none when switched off (tmac_hip_set_gemm_min_n(0)), an explicitly
// set threshold literally, else `fitted`, the caller's own default (setting 32, the knob's initial value, counts as "not set").
inline int gemm_min_rows(int fitted) { return g_knobs.gemm_min_n <= 0 ? INT_MAX : g_knobs.gemm_min_n != 32 ? g_knobs.gemm_min_n : fitted; }
// the LUT-image kind k_gemm_planes wants for this shape: row-wise for unified scales, else chunk-major
inline LutImage image_kind_for(const Shape& s) { return s.m_groups >= 1 ? IMG_ROWWISE : IMG_CHUNK; }
// The device layout of registered weights, which Shape spells as the pair (ts, lay): 16-table segments for the two-kernel path
// (k_gemv_lo), 8-table units in 16-row blocks (k_gemv_fused), or 8-table units in row quads (k_gemv_quad and the GEMMs).
enum Layout { L_LO, L_ROWBLOCK, L_QUAD };
inline Layout layout_of(const Shape& s) { return s.lay == 2 ? L_QUAD : s.ts == 8 ? L_ROWBLOCK : L_LO; }
inline void set_layout(Shape& s, Layout l) { s.ts = l == L_LO ? 16 : 8; s.lay = l == L_QUAD ? 2 : 0; }

// ---- kcfg (tmac_kcfg.cpp; callers hold g_mu) -----------------------------------------------------
// 1 = found, 0 = no section matches, -1 = several sections match and disagree on what the bytes mean
int find_cfg(int k, int n, int b, int bm_filter, int m_filter, tmac_kcfg* out, bool act_only = false);
void kcfg_clear_locked();

// ---- weights (tmac_weights.cpp) -------------------------------------------------------------------
int32_t make_shape(Shape& s, int Mw, int K, int bits, const tmac_kcfg* cfg);
size_t ref_weight_bytes(const Shape& s);
size_t ref_scale_elems(const Shape& s);
size_t dt_size(Dtype d);
int32_t register_impl(tmac_hip_weights** out, const void* A_ref, const void* scales_ref, bool src_on_device, int Mw, int K, int bits,
                      const tmac_kcfg* cfg, tmac_dtype_t host_float, tmac_dtype_t dev_float, void* stream);

// ---- workspace (tmac_workspace.cpp) ---------------------------------------------------------------
int32_t check_lut_shape(tmac_hip_workspace* ws, int K, int N, int ags);
LutBuildCaps lut_caps(const tmac_hip_workspace* ws);   // the knobs and the workspace as lut_build_plan reads them
// The launches of a plan of lut_build_plan (the only caller of launch_preprocess* and launch_lut_image): ws->held is cleared, and says what
// the plan says once the last launch was enqueued.  xf / perm_dev: the transform block / device permutation the request spoke of, or null.
int32_t lut_build(tmac_hip_workspace* ws, const LutBuildPlan& plan, const void* B_dev, tmac_dtype_t act_dtype, const XfRowsGateArgs* xf,
                  const int32_t* perm_dev, hipStream_t st);
// The fused entry point's workspace of this stream on the calling thread's device, large enough for K x N: one per (device, stream) --
// launches on one stream are ordered, two streams must not share LUT buffers -- grown on demand to the largest K and N seen.
int32_t stream_workspace(hipStream_t st, int K, int N, tmac_hip_workspace** out);
void release_fused_workspaces();    // tmac_hip_cache_clear; caller holds g_mu

// ---- dispatch (tmac_dispatch.cpp) -----------------------------------------------------------------
int32_t qgemm_impl(const tmac_hip_weights* w, const tmac_hip_workspace* ws, void* C_dev, tmac_dtype_t out_dtype, int N, int32_t* dump,
                   hipStream_t st);
// A fused call as one value: what tmac_hip_qgemm_fused_dev was handed.  A view: it owns nothing and allocates nothing; the lists live
// with the caller (or in a ChainRecOp, tmac_chain_host.h).  The split entry point wraps its matrix in a one-matrix call (B null) for the
// launch helpers it shares with the fused one.
struct FusedCall {
    const tmac_hip_weights* const* wl;
    int nmat;
    const void* B;
    tmac_dtype_t act;
    void* const* C;
    tmac_dtype_t out;
    int N;
    hipStream_t st;
    const Shape& s0() const { return wl[0]->s; }
    bool act_f16() const { return act == TMAC_F16; }
    bool out_f16() const { return out == TMAC_F16; }
    size_t out_bytes(int i) const { return (size_t)N * wl[i]->s.Mw * (out_f16() ? 2 : 4); }
};
int32_t fused_impl(const FusedCall& c, int32_t* dump, float* lut_tap);
// what a non-deferred, tap-less fused call is refused for (the per-matrix null checks and plan_fused): TMAC_HIP_OK, or fail(code, message).
// Pure: reads its argument and g_knobs.
int32_t fused_check(const FusedCall& c);
int32_t nulls_check(const FusedCall& c);      // a matrix or an output of the call is null (one of the doors' named checks)
// The fields of k_gemv_quad's / k_gemv_fused's argument block that the call decides (the door adds its own: taps, transform, permutation);
// returns the launch's row blocks (row quads in the QUAD layout) over all matrices.
int fill_fused_args(FusedArgs& fa, const FusedCall& c);
// Alignment of caller-owned device pointers: ACT_ALIGN, XFORM_ALIGN and misaligned are tmac_xform.h's; the GEMMs store four outputs at a
// time (fp32: 16 bytes, fp16: 8).
inline size_t out_align(tmac_dtype_t d) { return d == TMAC_F16 ? 8 : 16; }
// What k_gemv_quad's MFMA form with an in-kernel LUT build takes, as the set of conditions a matrix misses (0: it is served).  A door
// asks for the conditions in its scope and words its own refusal.
// The conditions: the reference-layout variant or the v_mqsad accumulate is selected | not registered in the QUAD layout, or its tiled
// kernel does not cover the configuration | fast-aggregation weights | gemv_quad_supported says no.
enum : unsigned { QM_REF_VARIANT = 1, QM_MQSAD_VARIANT = 2, QM_LAYOUT = 4, QM_FAST_AGG = 8, QM_SHAPE = 16 };
unsigned quad_mfma_misses(const tmac_hip_weights* w);

// ---- tuner (tmac_tuner.cpp) -----------------------------------------------------------------------
void tuned_config(const FusedArgs& fa, int total_q, int& ft, int& wpq);   // leaves ft / wpq alone when nothing is recorded

// ---- decode chain (tmac_chain_host.cpp) and deferred queue (tmac_defer.cpp) -----------------------------------------------------------
bool chain_recording();            // is the calling thread between tmac_hip_chain_begin and tmac_hip_chain_end?
bool chain_recording_independent();   // ... in a recording that was declared independent (tmac_hip_chain_begin_independent)?
void chain_clear_xform();          // drops a transform declared for the next recorded call (the call was rejected before it could be recorded)
int32_t chain_record(const FusedCall& c);
// deferred launches (tmac_hip_defer): true (and *rc set) when the call was queued instead of launched
bool defer_if_on(const FusedCall& c, int32_t* rc);
// Orders an entry point behind the calling thread's queue: flushes it when it is not empty and returns the flush's status (one
// vector::empty() otherwise).  First statement of every entry point that launches work or touches device memory for the caller; when it
// fails, nothing of the entry point is launched.  defer_flush takes the queue before it launches: the entry points it calls see none.
int32_t defer_barrier();
void defer_release_thread();       // frees the calling thread's cached recordings (tmac_hip_cache_clear)
void defer_reset_stats();          // zeroes the calling thread's tmac_hip_defer_stats counters (tmac_hip_reset_state)
void defer_forget_all();           // weights were freed / the library was reset: cached recordings of every thread are stale from now on
// true (and *rc set) when the calling thread is recording: the exchange step was noted, not executed
bool chain_record_gather_if_recording(const void* send_dev, void* recv_dev, size_t bytes_per_rank, int rank, int world, int32_t* rc);

// ---- host-pointer layer (tmac_hostptr.cpp) --------------------------------------------------------
void host_route_release();         // frees the layer's workspace, staging buffers and LUT memo (tiles / runs: tmac_hip_cache_clear)

}  // namespace tmac_host
