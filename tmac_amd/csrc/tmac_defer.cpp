// tmac_defer.cpp — the deferred queue (tmac_hip_defer / tmac_hip_flush): independent N = 1 calls launched together as one stream-mode chain.
#include "tmac_chain_host.h"
#include <algorithm>
#include <atomic>

using namespace tmac_host;

// ---------------------------------------------------------------------------------------------
// Deferred launches (include/tmac_hip.h: tmac_hip_defer / tmac_hip_flush).  A caller that does NOT record -- a backend hook called mat-mul by
// mat-mul -- still issues, between two synchronisation points, calls that do not depend on each other (q / k / v of a layer as separate
// calls; the projections of several sequences).  Launched one by one they run k_gemv_quad (0.25 of the HBM peak on the headline shape, a
// launch each); queued and flushed together they are ONE stream-mode launch (k_lut_images + k_gemv_stream).  The queue holds N = 1 calls
// whose inputs are resident: a call that reads or overwrites anything a queued call writes (or overwrites what one reads) flushes the
// queue first, so a batch never carries a dependence and never needs a hand-off.  The recording built from a batch is cached by the
// batch's signature (matrices, pointers, dtypes): a decode loop pays chain_build once per distinct batch.  What the persistent
// kernels do not cover (chain_build returns -1) is launched call by call at the flush, as if it had never been queued.
// Every other entry point that launches work or touches device memory for the caller goes behind the queue (defer_barrier: an
// unconditional flush, no range analysis -- none of them is a hot path).  A call is checked when it is queued (fused_check: what it
// would be refused for with deferral off), so a flush meets valid calls only; a flush launches ALL of them whatever fails on the way
// (a failed stream launch: its calls one by one) and leaves the queue empty.
// ---------------------------------------------------------------------------------------------
namespace {
struct DeferEntry {
    std::vector<ChainRecOp> sig;           // the batch it was built from (compared by ChainRecOp::same_call)
    std::vector<tmac_hip_chain*> chains;   // one stream-mode recording per configuration of the batch (bits, zero points, scale kind and dtype, output dtype)
    std::vector<std::vector<uint32_t>> chain_calls;   // ... and the calls of the batch it stands for (launched one by one when its launch fails)
    std::vector<uint32_t> singles;         // calls of the batch launched one by one (no persistent form, or alone in their configuration)
    unsigned long long used;
};
void defer_free_entry(DeferEntry& e, bool sync) {
    for (tmac_hip_chain* c : e.chains) {
        if (sync) (void)hipStreamSynchronize(c->last_stream);
        tmac_hip_chain_free(c);
    }
    e.chains.clear();
}
struct DeferState {
    bool on = false;
    std::vector<ChainRecOp> pending;
    hipStream_t stream = nullptr;
    std::vector<DeferEntry> cache;
    unsigned long long epoch = 0, tick = 0;
    unsigned long long n_flush = 0, n_hit = 0, n_stream = 0, n_chain = 0, n_single = 0;
    // (no destructor: a thread_local of the main thread is destroyed at process exit, when the HIP runtime may be gone -- the cached
    // recordings are released by tmac_hip_cache_clear / tmac_hip_reset_state on the owning thread, or with the process)
};
thread_local DeferState g_defer;
std::atomic<unsigned long long> g_defer_epoch{1};
constexpr size_t DEFER_MAX_BATCH = 256, DEFER_CACHE = 32, DEFER_MIN_STREAM = 3;

// tmac_hip_debug_defer_fail: is this launch attempt of a flush the one that was told to fail?  Host side only; one-shot.
bool defer_injected_failure() {
    if (g_knobs.defer_fail <= 0 || --g_knobs.defer_fail > 0) return false;
    return true;
}

int32_t defer_flush(hipStream_t st) {
    DeferState& D = g_defer;
    if (D.pending.empty()) return TMAC_HIP_OK;
    std::vector<ChainRecOp> batch;
    batch.swap(D.pending);
    ++D.n_flush;
    const unsigned long long ep = g_defer_epoch.load(std::memory_order_acquire);
    if (ep != D.epoch) {                      // weights were freed since: every cached recording may point at dead matrices
        for (DeferEntry& e : D.cache) defer_free_entry(e, false);
        D.cache.clear();
        D.epoch = ep;
    }
    auto same = [](const ChainRecOp& a, const ChainRecOp& b) { return a.same_call(b); };
    DeferEntry* hit = nullptr;
    for (DeferEntry& e : D.cache)
        if (e.sig.size() == batch.size() && std::equal(batch.begin(), batch.end(), e.sig.begin(), same)) { hit = &e; break; }
    if (hit) ++D.n_hit;
    else {
        // The calls of a batch are independent of each other (defer_if_on), so they may be regrouped: one recording per configuration
        // a persistent kernel is instantiated for -- a caller that mixes 2- and 4-bit matrices (qgemm.py:98-116 allows any mix) gets one
        // stream launch per width instead of a launch per call.
        DeferEntry ne;
        ne.sig = batch; ne.used = 0;
        std::vector<char> taken(batch.size(), 0);
        for (size_t i = 0; i < batch.size(); ++i) {
            if (taken[i]) continue;
            const tmac_hip_weights* wi = batch[i].w[0];
            std::vector<uint32_t> grp;
            for (size_t j = i; j < batch.size(); ++j) {
                const tmac_hip_weights* wj = batch[j].w[0];
                if (taken[j] || wj->s.bits != wi->s.bits || wj->s.zero_point != wi->s.zero_point || (wj->s.m_groups >= 1) != (wi->s.m_groups >= 1) ||
                    wj->sc_dtype != wi->sc_dtype || batch[j].out != batch[i].out) continue;
                taken[j] = 1; grp.push_back((uint32_t)j);
            }
            tmac_hip_chain* c = nullptr;
            // (a stream launch costs ~10 us before its first byte -- k_lut_images + the persistent kernel's ramp -- against ~4 us of launch and
            // ramp per stand-alone call: two calls are faster one by one, three break even, four win by a third: profiles/r06_stream_small_batches.txt)
            if (grp.size() >= DEFER_MIN_STREAM && !chain_recording()) {     // (a flush issued while the thread records launches call by call)
                std::vector<ChainRecOp> calls;
                for (uint32_t j : grp) calls.push_back(batch[j]);
                if (chain_build(calls, {}, &c) != TMAC_HIP_OK) c = nullptr;
                if (c && !c->stream) { tmac_hip_chain_free(c); c = nullptr; }    // (a batch carries no dependence: anything but a stream is not worth a persistent launch)
            }
            if (c) { ne.chains.push_back(c); ne.chain_calls.push_back(grp); }
            else ne.singles.insert(ne.singles.end(), grp.begin(), grp.end());
        }
        if (D.cache.size() >= DEFER_CACHE) {                    // evict the least recently used recording
            size_t v = 0;
            for (size_t i = 1; i < D.cache.size(); ++i) if (D.cache[i].used < D.cache[v].used) v = i;
            defer_free_entry(D.cache[v], true);
            D.cache.erase(D.cache.begin() + (long)v);
        }
        D.cache.push_back(ne);
        hit = &D.cache.back();
    }
    hit->used = ++D.tick;
    // Everything of the batch is launched whatever fails on the way; the first error of a call that was NOT launched is returned (a
    // stream launch that failed and whose calls then went out one by one is no error of the flush).
    int32_t first = TMAC_HIP_OK;
    const bool was_on = D.on;
    D.on = false;                                               // call by call, as if never queued
    auto single = [&](uint32_t j) {
        ++D.n_single;
        const int32_t rc = defer_injected_failure() ? fail(TMAC_HIP_E_RUNTIME, "deferred call: injected launch failure (tmac_hip_debug_defer_fail)")
                                                    : fused_impl(batch[j].call(st), nullptr, nullptr);
        if (rc != TMAC_HIP_OK && first == TMAC_HIP_OK) first = rc;
    };
    for (size_t g = 0; g < hit->chains.size(); ++g) {
        ++D.n_stream;
        const int32_t rc = defer_injected_failure() ? fail(TMAC_HIP_E_RUNTIME, "deferred batch: injected launch failure (tmac_hip_debug_defer_fail)")
                                                    : tmac_hip_chain_launch(hit->chains[g], st);
        if (rc != TMAC_HIP_OK) for (uint32_t j : hit->chain_calls[g]) single(j);
    }
    for (uint32_t j : hit->singles) single(j);
    D.on = was_on;
    return first;
}
}  // namespace

bool tmac_host::defer_if_on(const FusedCall& c, int32_t* rc) {
    DeferState& D = g_defer;
    if (!D.on) return false;
    *rc = TMAC_HIP_OK;
    if (c.N != 1) { *rc = defer_flush(D.stream); return *rc != TMAC_HIP_OK; }    // (ordered behind the queue; launched as usual -- unless the queue failed)
    // what the call would be refused for with deferral off: refused now, with that code and message, and the queue is left as it is
    if ((*rc = fused_check(c)) != TMAC_HIP_OK) return true;
    const ChainRecOp op(c);
    // a dependence on the queue (RAW: reads a queued output; WAR / WAW: writes what a queued call reads or writes), another stream, or a
    // full queue: the queue goes first
    bool must_flush = !D.pending.empty() && (c.st != D.stream || D.pending.size() >= DEFER_MAX_BATCH);
    const Range in = act_range(op);
    for (size_t j = 0; j < D.pending.size() && !must_flush; ++j) {
        const ChainRecOp& p = D.pending[j];
        const Range pin = act_range(p);
        for (size_t m = 0; m < p.C.size() && !must_flush; ++m) {
            const Range po = out_range(p, m, p.out);
            if (overlap(in, po)) must_flush = true;
            for (size_t k = 0; k < op.C.size(); ++k) if (overlap(out_range(op, k, op.out), po)) must_flush = true;
        }
        for (size_t k = 0; k < op.C.size(); ++k) if (overlap(out_range(op, k, op.out), pin)) must_flush = true;
    }
    if (must_flush && (*rc = defer_flush(D.stream)) != TMAC_HIP_OK) return true;
    D.stream = c.st;
    D.pending.push_back(op);
    return true;
}
int32_t tmac_host::defer_barrier() { return g_defer.pending.empty() ? TMAC_HIP_OK : defer_flush(g_defer.stream); }
void tmac_host::defer_forget_all() { g_defer_epoch.fetch_add(1, std::memory_order_acq_rel); }
void tmac_host::defer_reset_stats() {             // the calling thread's tmac_hip_defer_stats counters (tmac_hip_reset_state)
    DeferState& D = g_defer;
    D.n_flush = D.n_hit = D.n_stream = D.n_chain = D.n_single = 0;
}
void tmac_host::defer_release_thread() {          // the calling thread's cached recordings (nothing of them may be in flight: the caller has synchronised)
    DeferState& D = g_defer;
    for (DeferEntry& e : D.cache) defer_free_entry(e, false);
    D.cache.clear();
}

extern "C" int32_t tmac_hip_defer(int on) {
    DeferState& D = g_defer;
    const int32_t rc = on ? TMAC_HIP_OK : defer_barrier();      // (the queue is empty afterwards whatever the flush returns)
    D.on = on != 0;
    return rc;
}
extern "C" int32_t tmac_hip_flush(void* stream) {
    (void)stream;                                               // (the queue remembers the stream its calls were issued on)
    return defer_flush(g_defer.stream);
}
extern "C" int32_t tmac_hip_debug_defer_fail(int nth) {
    g_knobs.defer_fail = nth > 0 ? nth : 0;
    return TMAC_HIP_OK;
}
extern "C" int32_t tmac_hip_defer_stats(uint64_t* flushes, uint64_t* cache_hits, uint64_t* stream_launches, uint64_t* single_calls) {
    const DeferState& D = g_defer;
    if (flushes) *flushes = D.n_flush;
    if (cache_hits) *cache_hits = D.n_hit;
    if (stream_launches) *stream_launches = D.n_stream;
    if (single_calls) *single_calls = D.n_single;
    return TMAC_HIP_OK;
}
