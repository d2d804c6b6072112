// tmac_chain_host.h — what the host-side units of the persistent decode chain share: tmac_chain_host.cpp records and builds a chain,
// tmac_chain_launch.cpp runs and inspects it, tmac_defer.cpp builds chains from queued calls.  Nothing here is exported.
#pragma once
#include "tmac_host.h"

struct tmac_hip_chain {
    std::vector<tmac::ChainOp> ops;
    tmac::ChainOp* d_ops = nullptr;
    unsigned* ctl = nullptr;
    // hand-off images of all consumed outputs: ONE arena (same layout on every rank of a row-sharded chain: a peer's address of
    // a granule is its arena base plus the local offset)
    void* arena = nullptr;
    size_t arena_bytes = 0;
    unsigned long long layout_hash = 0;
    int rank = 0, world = 1;
    std::vector<void*> peers;         // the other ranks' arenas, mapped through IPC (rank order, self skipped)
    bool connected = false;
    int bits = 0, zp = 0, sc_f16 = 0, out_f16 = 0;
    int sm = 0;                       // 0 per-group scales, 2 unified scale (k_decode_chain's SM)
    int grid = 0, buf_u4 = 0;
    size_t lds_bytes = 0;
    unsigned long long* stamps = nullptr;
    int32_t* tap = nullptr;           // parity tap (tmac_hip_chain_set_tap): caller's device buffer; per-op offsets (ints) on the device
    unsigned long long* d_tap_off = nullptr;
    size_t bytes = 0;                 // algorithmic weight + scale bytes of one launch
    int xforms = 0, carry_floats = 0;    // some op carries a vector transform; LDS floats of the kept vector
    int gates = 0;                       // some GLU of the chain has a gate other than silu (ChainArgs::gates)
    int tmp_floats = 0, gam_floats = 0, ext_floats = 0, carry_K = 0;   // LDS floats of an op's own transform vector / norm weights; K of the latest kept vector
    int poll_sleep = 8, poll_delay = 4, issue_first = -1, poll_mode = 0, poll_grid = 0;   // read from the environment once, when the chain is built
    hipStream_t last_stream = nullptr;   // stream of the most recent launch (in-flight guard)
    bool launched = false;
    // stream mode (tmac_stream.hip): no op consumes another's output -- k_lut_images builds every op's tables once into `images`
    // (one image per op, the layout of the LDS LUT buffer), k_gemv_stream walks the ops with the tables prebuilt
    bool stream = false;
    void* images = nullptr;
    int max_nst = 0;
    const int* roles = nullptr;       // stream mode: the lookup waves' role records (device, behind the images), then the classes' visit counts
    const int* nvis = nullptr;
    int ncls = 1, vmax = 0;           // the schedule: classes of row ranges, records per class
    bool qw = false;                  // k_gemv_stream's quarter-walk form (rows dealt in groups of four quads: q_end / q_per / q_extra of the ops count groups)
    int nsplit = 1;                   // workgroups per row range (two share a CU and take alternate ops when LDS and registers allow)
    // act-order ops (a recording declared independent, tmac_hip_chain_begin_independent): perms[op] is the K permutation the op's matrices
    // carry (null: a plain op) -- owned here, so that the device arrays k_lut_images' gather form reads outlive the handles and the
    // caller's tmac_hip_kperm -- and d_perms their device pointers, one per op, uploaded beside d_ops; both empty / null without such an op
    bool has_perm = false;
    std::vector<std::shared_ptr<KPermData>> perms;
    const int32_t** d_perms = nullptr;
    int g2 = 0;                       // 1 iff some op has scale groups of 64: both launchers then run the instances with two scale groups per lane
                                      // and item (tmac_chain_core.h, G2); a recording without such an op launches the kernels it always did
};

namespace tmac_host {

// one noted tmac_hip_qgemm_fused_dev call (N = 1): of a recording, or of the deferred queue
struct ChainRecOp {
    std::vector<const tmac_hip_weights*> w;
    const void* B;
    std::vector<void*> C;
    tmac_dtype_t act, out;
    XfSpec xf;                       // vector transform of the activations, resolved (tmac_xform.h; kind 0: none)
    std::shared_ptr<KPermData> perm; // the K permutation all matrices of the call carry (act-order; a declared-independent recording only), or null
    ChainRecOp() = default;
    explicit ChainRecOp(const FusedCall& c) : w(c.wl, c.wl + c.nmat), B(c.B), C(c.C, c.C + c.nmat), act(c.act), out(c.out) {}
    // ... and back: the call as a view over this op's own lists
    FusedCall call(hipStream_t st) const { return FusedCall{w.data(), (int)w.size(), B, act, C.data(), out, 1, st}; }
    // the fields that make two noted calls the same call (a deferred batch's signature is its calls)
    bool same_call(const ChainRecOp& o) const { return B == o.B && act == o.act && out == o.out && w == o.w && C == o.C && perm == o.perm; }
};
// an exchange step noted while recording: recv = all-gather over the ranks of send (rank r's bytes at r * bytes)
struct ChainRecGather {
    const void* send;
    const void* recv;
    size_t bytes;
    int rank, world;
    size_t pos;                       // number of calls recorded before it
};

// half-open byte ranges
struct Range { const char* lo; const char* hi; };
inline bool overlap(const Range& a, const Range& b) { return a.lo < b.hi && b.lo < a.hi; }
// what a call reads as activations, and what it writes for matrix m as values of dtype `out`
inline Range act_range(const ChainRecOp& r) { return Range{(const char*)r.B, (const char*)r.B + (size_t)r.w[0]->s.K * (r.act == TMAC_F32 ? 4 : 2)}; }
inline Range out_range(const ChainRecOp& r, size_t m, tmac_dtype_t out) {
    return Range{(const char*)r.C[m], (const char*)r.C[m] + (size_t)r.w[m]->s.Mw * (out == TMAC_F16 ? 2 : 4)};
}

// Builds the chain of the calls `rec` (and the exchange steps noted between them): tmac_hip_chain_end's return codes and messages.
// declared: the recording was declared independent when it began -- a stream chain or TMAC_HIP_E_ARG, never k_decode_chain.
int32_t chain_build(const std::vector<ChainRecOp>& rec, const std::vector<ChainRecGather>& gat, tmac_hip_chain** out, bool declared = false);

}  // namespace tmac_host
