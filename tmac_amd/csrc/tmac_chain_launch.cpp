// tmac_chain_launch.cpp — running and inspecting a built decode chain: launch, the IPC exchange of row-sharded chains, status, info, taps, stamps.
#include "tmac_chain_host.h"

using namespace tmac_host;

extern "C" int32_t tmac_hip_chain_launch(tmac_hip_chain* c, void* stream) {
    bind_thread_device();
    const int32_t brc = defer_barrier();       // behind the calling thread's deferred queue (the chain may read or overwrite what a queued call writes or reads)
    if (brc) return brc;
    if (!c) return fail(TMAC_HIP_E_ARG, "null chain");
    hipStream_t st = (hipStream_t)stream;
    // One launch of a chain at a time (its hand-off buffers and control words are per chain): launches on ONE stream are
    // ordered by the stream; a launch on another stream is refused while the previous one may still be running.
    if (c->launched && st != c->last_stream && hipStreamQuery(c->last_stream) != hipSuccess) {
        (void)hipGetLastError();
        return fail(TMAC_HIP_E_ARG, "the chain is still in flight on another stream: synchronise it first, or record one chain per stream");
    }
    if (!c->connected) return fail(TMAC_HIP_E_ARG, "a row-sharded chain must be connected to its peers first (tmac_hip_chain_export / tmac_hip_chain_connect)");
    if (c->stream) {
        hipError_t e = launch_lut_images(c->d_ops, c->d_perms, (int)c->ops.size(), c->max_nst, c->sm, c->sc_f16 != 0, st);
        if (e != hipSuccess) return fail(TMAC_HIP_E_RUNTIME, "LUT image launch: %s", hipGetErrorString(e));
        StreamArgs sa;
        memset(&sa, 0, sizeof(sa));
        sa.ops = c->d_ops; sa.nops = (int)c->ops.size(); sa.out_f16 = c->out_f16; sa.buf_u4 = c->buf_u4; sa.nsplit = c->nsplit; sa.roles = c->roles; sa.stamps = c->stamps;
        sa.ncls = c->ncls; sa.vmax = c->vmax; sa.nvis = c->nvis; sa.tap = c->tap; sa.tap_off = c->d_tap_off;
        e = launch_gemv_stream(sa, c->bits, c->zp != 0, c->sc_f16 != 0, c->sm, c->qw, c->g2 != 0, c->grid, c->lds_bytes, st);
        if (e != hipSuccess) return fail(TMAC_HIP_E_RUNTIME, "stream launch: %s", hipGetErrorString(e));
        c->last_stream = st; c->launched = true;
        return TMAC_HIP_OK;
    }
    ChainArgs a;
    memset(&a, 0, sizeof(a));
    a.ops = c->d_ops; a.nops = (int)c->ops.size(); a.ctl = c->ctl; a.out_f16 = c->out_f16;
    a.arena_base = reinterpret_cast<unsigned long long>(c->arena); a.arena_half = c->arena_bytes;
    a.npeer = (int)c->peers.size();
    for (int p = 0; p < a.npeer; ++p) a.peer_base[p] = reinterpret_cast<unsigned long long>(c->peers[p]);
    a.spin_limit = g_knobs.chain_spin_limit; a.buf_u4 = c->buf_u4; a.stamps = c->stamps;
    a.xforms = c->xforms; a.gates = c->gates; a.carry_floats = c->carry_floats; a.tmp_floats = c->tmp_floats; a.gam_floats = c->gam_floats; a.ext_floats = c->ext_floats;
    {   // measurement only (tools/gpu): run a chain WITHOUT transforms through the kernel instance that knows them
        static const int force_xf = [] { const char* e = getenv("TMAC_HIP_CHAIN_FORCE_XF"); return e && e[0] == '1' ? 1 : 0; }();
        if (force_xf) a.xforms = 1;
    }
    if (c->tap) { a.tap = c->tap; a.tap_off = c->d_tap_off; a.xforms = 1; }      // the tap has an instance of its own (XF + TAP), launch_decode_chain_b*
    a.poll_sleep = c->poll_sleep; a.poll_delay = c->poll_delay; a.issue_first = c->issue_first; a.poll_mode = c->poll_mode; a.poll_grid = c->poll_grid;
    hipError_t e = launch_decode_chain(a, c->bits, c->zp != 0, c->sc_f16 != 0, c->sm, c->g2 != 0, c->grid, c->lds_bytes, st);
    if (e == hipErrorInvalidValue) return fail(TMAC_HIP_E_NOMATCH, "no decode-chain kernel for this configuration");
    if (e != hipSuccess) return fail(TMAC_HIP_E_RUNTIME, "decode chain launch: %s", hipGetErrorString(e));
    c->last_stream = st; c->launched = true;
    return TMAC_HIP_OK;
}

// ---- row-sharded chains: the ranks exchange the IPC handles of their hand-off arenas (any transport: MPI, torch.distributed, a
// file), then every producer stores its granules into all of them ----
struct ChainBlob {
    hipIpcMemHandle_t handle;
    unsigned long long arena_bytes, layout_hash;
    int rank, world;
};
static_assert(sizeof(ChainBlob) <= TMAC_HIP_CHAIN_BLOB_BYTES, "blob size");

extern "C" int32_t tmac_hip_chain_export(const tmac_hip_chain* c, void* blob_out) {
    if (!c || !blob_out) return fail(TMAC_HIP_E_ARG, "null argument");
    if (!c->arena) return fail(TMAC_HIP_E_ARG, "the chain hands nothing over");
    ChainBlob b;
    memset(&b, 0, sizeof(b));
    HIP_TRY(hipIpcGetMemHandle(&b.handle, c->arena));
    b.arena_bytes = 2 * c->arena_bytes; b.layout_hash = c->layout_hash; b.rank = c->rank; b.world = c->world;
    memset(blob_out, 0, TMAC_HIP_CHAIN_BLOB_BYTES);
    memcpy(blob_out, &b, sizeof(b));
    return TMAC_HIP_OK;
}

extern "C" int32_t tmac_hip_chain_connect(tmac_hip_chain* c, const void* blobs, int world) {
    if (!c || !blobs) return fail(TMAC_HIP_E_ARG, "null argument");
    if (world != c->world) return fail(TMAC_HIP_E_ARG, "the chain was recorded for %d ranks, %d blobs given", c->world, world);
    if (c->connected && c->world > 1) return fail(TMAC_HIP_E_ARG, "the chain is already connected");
    bind_thread_device();
    for (int r = 0; r < world; ++r) {
        ChainBlob b;
        memcpy(&b, (const char*)blobs + (size_t)r * TMAC_HIP_CHAIN_BLOB_BYTES, sizeof(b));
        if (b.rank != r || b.world != world || b.arena_bytes != 2 * c->arena_bytes || b.layout_hash != c->layout_hash)
            return fail(TMAC_HIP_E_ARG, "rank %d recorded a different chain (its blob does not match this rank's hand-off layout)", r);
        if (r == c->rank) continue;
        void* p = nullptr;
        hipError_t e = hipIpcOpenMemHandle(&p, b.handle, hipIpcMemLazyEnablePeerAccess);
        if (e != hipSuccess) {
            for (void* q : c->peers) if (q) (void)hipIpcCloseMemHandle(q);
            c->peers.clear();
            return fail(TMAC_HIP_E_RUNTIME, "hipIpcOpenMemHandle of rank %d's hand-off arena: %s", r, hipGetErrorString(e));
        }
        c->peers.push_back(p);
    }
    c->connected = true;
    return TMAC_HIP_OK;
}

// After the stream has been synchronised: 0 = every hand-off completed; otherwise the error word of the first wave that
// gave up (bit 31 | op << 8 | wave) -- the outputs are then invalid.  Clears the word and re-arms the chain.
extern "C" int32_t tmac_hip_chain_status(tmac_hip_chain* c, uint32_t* error_word) {
    if (!c || !error_word) return fail(TMAC_HIP_E_ARG, "null argument");
    unsigned ctl[4];
    HIP_TRY(hipMemcpy(ctl, c->ctl, sizeof(ctl), hipMemcpyDeviceToHost));
    *error_word = ctl[2];
    if (ctl[2] || ctl[1]) {
        // A launch that gave up still ran to its end and advanced the generation like any other (every wait is bounded, the last
        // workgroup out advances): the generation stays in step with the peers of a row-sharded chain, which count launches the same
        // way -- re-arming one rank here would leave it a generation apart from its peers for good.  Only the error word (and a partial
        // exit count, should the launch have been killed from outside) is cleared.
        // A partial exit count means the launch never advanced the generation: the next launch reuses it and the same arena half, where
        // the granules the dead launch already published carry a matching tag.  They are wiped (tag 0 is never a generation), so the
        // next launch waits for data of its own.
        if (ctl[1] && c->world > 1)
            // ... on ONE GPU.  A row-sharded launch that died part-way has also stored granules into the peers' arenas under a generation the
            // peers have meanwhile left behind: the ranks are a generation apart and no local wipe repairs that
            return fail(TMAC_HIP_E_RUNTIME, "a row-sharded chain was interrupted inside a launch (%u of its workgroups exited): the ranks' generations differ now -- "
                                            "free the chain on every rank, record and connect it again", ctl[1]);
        if (ctl[1] && c->arena) HIP_TRY(hipMemset(c->arena, 0, 2 * c->arena_bytes));
        const unsigned fresh[4] = {ctl[0], 0u, 0u, 0u};
        HIP_TRY(hipMemcpy(c->ctl, fresh, sizeof(fresh), hipMemcpyHostToDevice));
    }
    return TMAC_HIP_OK;
}

extern "C" int32_t tmac_hip_chain_info(const tmac_hip_chain* c, int op, int32_t* nops, int32_t* wpq, int32_t* grid, size_t* bytes) {
    if (!c) return fail(TMAC_HIP_E_ARG, "null chain");
    if (nops) *nops = (int32_t)c->ops.size();
    if (grid) *grid = c->grid;
    if (bytes) *bytes = c->bytes;
    if (wpq) {
        if (op < 0 || op >= (int)c->ops.size()) return fail(TMAC_HIP_E_ARG, "op index out of range");
        *wpq = c->ops[op].wpq;
    }
    return TMAC_HIP_OK;
}

// Parity tap of the persistent kernels (include/tmac_hip.h): the integers of every recorded call as they enter the float part.
// off[op]: where op's integers start in the tap buffer; off[nops]: the buffer's size
static std::vector<unsigned long long> tap_offsets(const tmac_hip_chain* c) {
    std::vector<unsigned long long> off(c->ops.size() + 1, 0);
    for (size_t i = 0; i < c->ops.size(); ++i)
        off[i + 1] = off[i] + (unsigned long long)4 * c->ops[i].total_q * (c->sm == 2 ? c->bits : c->ops[i].G);
    return off;
}
extern "C" int32_t tmac_hip_chain_tap_layout(const tmac_hip_chain* c, int op, size_t* offset_ints, size_t* count_ints) {
    if (!c) return fail(TMAC_HIP_E_ARG, "null chain");
    if (op < 0 || op > (int)c->ops.size()) return fail(TMAC_HIP_E_ARG, "op index out of range");
    const std::vector<unsigned long long> off = tap_offsets(c);
    if (offset_ints) *offset_ints = (size_t)off[op];
    if (count_ints) *count_ints = op < (int)c->ops.size() ? (size_t)(off[op + 1] - off[op]) : 0;
    return TMAC_HIP_OK;
}
extern "C" int32_t tmac_hip_chain_set_tap(tmac_hip_chain* c, int32_t* dev_buffer) {
    if (!c) return fail(TMAC_HIP_E_ARG, "null chain");
    if (!dev_buffer) { c->tap = nullptr; return TMAC_HIP_OK; }
    for (const ChainOp& o : c->ops)
        if (o.epi) return fail(TMAC_HIP_E_NOMATCH, "the tap does not cover calls whose row quads are dealt in gate / up pairs (GLU in the producer)");
    bind_thread_device();
    if (!c->d_tap_off) {
        const std::vector<unsigned long long> off = tap_offsets(c);
        if (hipMalloc((void**)&c->d_tap_off, off.size() * sizeof(unsigned long long)) != hipSuccess ||
            hipMemcpy(c->d_tap_off, off.data(), off.size() * sizeof(unsigned long long), hipMemcpyHostToDevice) != hipSuccess)
            return fail(TMAC_HIP_E_RUNTIME, "tap offsets: allocation failed");
    }
    c->tap = dev_buffer;
    return TMAC_HIP_OK;
}

// profiling aid: s_memrealtime stamps [ops][workgroups][8] of wave 0 (layout: tmac_chain.h)
extern "C" int32_t tmac_hip_chain_set_stamps(tmac_hip_chain* c, unsigned long long* dev_buffer) {
    if (!c) return fail(TMAC_HIP_E_ARG, "null chain");
#ifndef TMAC_STREAM_STAMPS
    // k_gemv_stream writes stamps in profiling builds only, and then in ITS layout ([workgroups][lookup waves][8], tmac_chain.h), not the
    // [calls][workgroups][8] documented for k_decode_chain: a buffer sized for the latter would be overrun
    if (c->stream && dev_buffer) return fail(TMAC_HIP_E_NOMATCH, "stamps of a stream-mode chain exist in -DTMAC_STREAM_STAMPS builds only (layout: StreamArgs::stamps)");
#endif
    if (!c->stream && dev_buffer && !TMAC_CHAIN_STAMPS)
        return fail(TMAC_HIP_E_NOMATCH, "stamps of k_decode_chain exist in -DTMAC_CHAIN_STAMPS=1 builds of the library only (tools/build_variant.sh)");
    c->stamps = dev_buffer;
    return TMAC_HIP_OK;
}

extern "C" int32_t tmac_hip_chain_threads(void) { return CHAIN_FT; }

extern "C" int32_t tmac_hip_chain_is_stream(const tmac_hip_chain* c) { return c && c->stream ? (c->qw ? 2 : 1) : 0; }
