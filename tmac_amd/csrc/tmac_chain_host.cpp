// tmac_chain_host.cpp — recording and building the persistent decode chain (kernels: tmac_chain.hip, tmac_stream.hip).
#include "tmac_chain_host.h"
#include "tmac_chain_indep.h"
#include <algorithm>
#include <array>
#include <memory>
#include <optional>

using namespace tmac_host;

// ---------------------------------------------------------------------------------------------
// Persistent decode chain (tmac_chain.hip): the fused calls of one decoded token recorded once, then executed by ONE
// launch.  Recording mirrors stream capture: between tmac_hip_chain_begin() and tmac_hip_chain_end() the calling thread's
// tmac_hip_qgemm_fused_dev calls (N = 1) are noted instead of launched; data flow is inferred from pointer identity (an
// op whose activation pointer equals an earlier op's output pointer consumes that output inside the launch).
// ---------------------------------------------------------------------------------------------
static thread_local std::vector<ChainRecOp>* g_chain_rec = nullptr;
static thread_local std::vector<ChainRecGather>* g_chain_gat = nullptr;
static thread_local std::optional<XfSpec> g_chain_xf;               // the transform declared for the next recorded call, resolved (tmac_xform.h)
// The recording was declared independent when it began (tmac_hip_chain_begin_independent): it ends as a stream chain or not at all, so
// transforms and exchange steps are refused as they come, and calls on act-order handles -- whose gather only k_lut_images has -- are noted.
static thread_local bool g_chain_declared = false;
bool tmac_host::chain_recording() { return g_chain_rec != nullptr; }
bool tmac_host::chain_recording_independent() { return g_chain_rec != nullptr && g_chain_declared; }
void tmac_host::chain_clear_xform() { g_chain_xf.reset(); }

int32_t tmac_host::chain_record(const FusedCall& c) {
    // (a rejected call must not leave its transform pending for the next recorded call)
    if (c.N != 1) { chain_clear_xform(); return fail(TMAC_HIP_E_NOMATCH, "a decode chain records N = 1 calls only"); }
    const int32_t nrc = nulls_check(c);
    if (nrc) { chain_clear_xform(); return nrc; }
    ChainRecOp op(c);
    op.perm = c.wl[0]->kperm;           // (fused_impl: all matrices carry it, or none does; non-null in a declared-independent recording only)
    op.xf = g_chain_xf.value_or(XfSpec{});
    chain_clear_xform();
    g_chain_rec->push_back(op);
    return TMAC_HIP_OK;
}

// A vector transform for the NEXT recorded call (include/tmac_hip.h): validated when the chain is built.
extern "C" int32_t tmac_hip_chain_xform(const tmac_hip_xform* xf) {
    if (!g_chain_rec) return fail(TMAC_HIP_E_ARG, "no chain is being recorded on this thread");
    if (g_chain_declared) return fail(TMAC_HIP_E_ARG, "this recording was declared independent (tmac_hip_chain_begin_independent): its calls carry no vector transform");
    if (!xf) return fail(TMAC_HIP_E_ARG, "null transform");
    XfSpec spec;
    const int32_t rc = xf_resolve(xf, XF_SITE_CHAIN, &spec);
    if (rc) return rc;
    g_chain_xf = spec;
    return TMAC_HIP_OK;
}

static int32_t chain_begin(bool declared) {
    if (g_chain_rec) return fail(TMAC_HIP_E_ARG, "a chain is already being recorded on this thread");
    g_chain_rec = new std::vector<ChainRecOp>();
    g_chain_gat = new std::vector<ChainRecGather>();
    g_chain_declared = declared;
    chain_clear_xform();
    return TMAC_HIP_OK;
}
extern "C" int32_t tmac_hip_chain_begin(void) { return chain_begin(false); }
// ... declared independent (include/tmac_hip.h): tmac_hip_chain_end builds stream mode or fails
extern "C" int32_t tmac_hip_chain_begin_independent(void) { return chain_begin(true); }

// Ends a recording without building anything (a caller whose recording hit an error: the thread is free to launch calls again).
extern "C" int32_t tmac_hip_chain_abort(void) {
    if (!g_chain_rec) return TMAC_HIP_OK;
    delete g_chain_rec;
    delete g_chain_gat;
    g_chain_rec = nullptr;
    g_chain_gat = nullptr;
    g_chain_declared = false;
    chain_clear_xform();
    return TMAC_HIP_OK;
}

// Ends the recording (whatever comes out: the thread launches calls again) and builds the chain of what was noted.
extern "C" int32_t tmac_hip_chain_end(tmac_hip_chain** out) {
    if (!g_chain_rec) return fail(TMAC_HIP_E_ARG, "no chain is being recorded on this thread");
    std::vector<ChainRecOp> rec;
    std::vector<ChainRecGather> gat;
    rec.swap(*g_chain_rec);
    gat.swap(*g_chain_gat);
    delete g_chain_rec;
    delete g_chain_gat;
    g_chain_rec = nullptr;
    g_chain_gat = nullptr;
    const bool declared = g_chain_declared;
    g_chain_declared = false;
    if (!out) return fail(TMAC_HIP_E_ARG, "null argument");
    return chain_build(rec, gat, out, declared);
}

// The exchange step of a row-sharded chain, noted instead of executed (tmac_hip_comm_allgather calls this while the thread
// records): the calls that read recv_dev afterwards consume, inside the launch, what every rank's producer of send_dev publishes.
extern "C" int32_t tmac_hip_chain_record_gather(const void* send_dev, void* recv_dev, size_t bytes_per_rank, int rank, int world) {
    if (!g_chain_rec) return fail(TMAC_HIP_E_ARG, "no chain is being recorded on this thread");
    if (g_chain_declared) return fail(TMAC_HIP_E_ARG, "this recording was declared independent (tmac_hip_chain_begin_independent): it takes no exchange step");
    if (!send_dev || !recv_dev || !bytes_per_rank || world < 1 || world > 8 || rank < 0 || rank >= world)
        return fail(TMAC_HIP_E_ARG, "bad gather (1..8 ranks)");
    g_chain_gat->push_back(ChainRecGather{send_dev, recv_dev, bytes_per_rank, rank, world, g_chain_rec->size()});
    return TMAC_HIP_OK;
}
bool tmac_host::chain_record_gather_if_recording(const void* send_dev, void* recv_dev, size_t bytes_per_rank, int rank, int world, int32_t* rc) {
    if (!g_chain_rec) return false;
    *rc = tmac_hip_chain_record_gather(send_dev, recv_dev, bytes_per_rank, rank, world);
    return true;
}

static int chain_pick_wpq(int total_q, int nst, int grid, int nwv = CHAIN_NWV) {
    int best = 1;
    long best_cost = 1L << 60;
    for (int wpq = 1; wpq <= 4; ++wpq) {          // the combinations k_gemv_quad is instantiated for with this many threads
        if (nwv % wpq || (wpq > 1 && wpq > nst)) continue;
        const long ipi = nwv / wpq;
        const long cnt = (total_q + grid - 1) / grid;               // quads of the busiest workgroup (balanced contiguous ranges)
        const long iters = (cnt + ipi - 1) / ipi;
        const long steps = (nst + wpq - 1) / wpq;
        if (iters * steps < best_cost) { best_cost = iters * steps; best = wpq; }     // ties: fewer waves per quad (no LDS combine)
    }
    return best;
}

extern "C" int32_t tmac_hip_chain_free(tmac_hip_chain* c) {
    if (!c) return TMAC_HIP_OK;
    const int32_t brc = defer_barrier();       // (the calling thread's queued calls go first; the chain is freed whatever they return)
    for (void* p : c->peers) if (p) (void)hipIpcCloseMemHandle(p);
    if (c->arena) (void)hipFree(c->arena);
    if (c->images) (void)hipFree(c->images);
    if (c->d_tap_off) (void)hipFree(c->d_tap_off);
    if (c->d_ops) (void)hipFree(c->d_ops);
    if (c->d_perms) (void)hipFree(c->d_perms);
    if (c->ctl) (void)hipFree(c->ctl);
    delete c;
    return brc;
}

static void set_wpq(ChainOp& o, int wpq, int nwv) {   // waves per row quad of an op of nwv lookup waves, and what the kernels derive from it
    o.wpq = wpq;
    o.ipi = nwv / wpq;
    o.wpq_inv = (65536 + wpq - 1) / wpq;
    o.ipi_inv = (65536 + o.ipi - 1) / o.ipi;
}

// ---- the stream schedule (tmac_chain.h, StreamArgs): a pure function of the calls' sizes, so that it can be tested without a device ----
// items[i]: lookup items of call i; grid row ranges in ncls classes of consecutive ranges (class c = ranges ceil(c grid / ncls) ..).  Every
// call gets an aligned block of blk_w[i] classes starting at class blk_lo[i]: a call that would give a range fewer than `target` items at
// full width is dealt to 1 / n of the ranges (n a power of two <= cap); the cap that gives the shortest modelled launch is taken (a lone
// call keeps all ranges).  Calls go to the least loaded block, widest blocks first and larger calls first (lpt), or in recorded order.
// visits[c]: the calls class c visits, in visiting order.
static int cls_lo(int cl, int grid, int ncls) { return (cl * grid + ncls - 1) / ncls; }     // the first row range of class cl
static void stream_schedule(const std::vector<double>& items, int grid, int ncls, int target, bool lpt, std::vector<int>& blk_lo, std::vector<int>& blk_w,
                            std::vector<std::vector<int>>& visits) {
    const int nop = (int)items.size();
    const double visit_fixed = 8.0;                                    // a visit's fixed cost in items (model only)
    blk_lo.assign(nop, 0); blk_w.assign(nop, ncls);
    visits.assign(ncls, std::vector<int>());
    double best_span = 0;
    int best_cap = 0;
    for (int pass = 0; pass < 2; ++pass) {
        for (int cap = ncls; cap >= 1; cap >>= 1) {
            if (pass == 1 && cap != best_cap) continue;
            std::vector<double> load(ncls, 0.0);
            std::vector<std::vector<int>> vis(ncls);
            // widest blocks first, larger calls first (longest-processing-time order: the calls are independent, so a class may visit
            // them in any order): in recorded order the classes of a llama-2-7B token ended 3 % apart, BitNet-3B's 8 % -- the launch
            // lasts as long as its most loaded class; in this order 0 % / 2 % (the same model)
            std::vector<int> order(nop), wof(nop);
            for (int i = 0; i < nop; ++i) {
                int n = 1;
                while (n < cap && items[i] * n / grid < target) n <<= 1;
                order[i] = i; wof[i] = ncls / n;
            }
            if (lpt)
                std::stable_sort(order.begin(), order.end(), [&](int x, int y) {
                    if (wof[x] != wof[y]) return wof[x] > wof[y];
                    return items[x] > items[y];
                });
            for (int oi = 0; oi < nop; ++oi) {
                const int i = order[oi], w = wof[i];
                int bb = 0;
                double bl = 1e300;
                for (int b0 = 0; b0 + w <= ncls; b0 += w) {
                    double m = 0;
                    for (int k = b0; k < b0 + w; ++k) m = load[k] > m ? load[k] : m;
                    if (m < bl) { bl = m; bb = b0; }
                }
                const int wg = cls_lo(bb + w, grid, ncls) - cls_lo(bb, grid, ncls);
                for (int k = bb; k < bb + w; ++k) { load[k] += visit_fixed + items[i] / wg; vis[k].push_back(i); }
                if (pass == 1) { blk_lo[i] = bb; blk_w[i] = w; }
            }
            double span = 0;
            for (int k = 0; k < ncls; ++k) span = load[k] > span ? load[k] : span;
            if (pass == 0 && (best_cap == 0 || span < best_span * 0.999)) { best_span = span; best_cap = cap; }
            if (pass == 1) visits.swap(vis);
        }
    }
}
// test hook (no device needed): the schedule of n calls with the given item counts; out_lo / out_w [n], out_load [ncls] = items per range of every class
extern "C" int32_t tmac_hip_debug_stream_schedule(const double* items, int n, int grid, int ncls, int target, int lpt, int32_t* out_lo, int32_t* out_w, double* out_load) {
    if (!items || n < 1 || grid < 1 || ncls < 1 || ncls > 16 || (ncls & (ncls - 1)) || ncls > grid || !out_lo || !out_w) return fail(TMAC_HIP_E_ARG, "bad schedule query");
    std::vector<double> it(items, items + n);
    std::vector<int> lo, w;
    std::vector<std::vector<int>> vis;
    stream_schedule(it, grid, ncls, target, lpt != 0, lo, w, vis);
    for (int i = 0; i < n; ++i) { out_lo[i] = lo[i]; out_w[i] = w[i]; }
    if (out_load)
        for (int k = 0; k < ncls; ++k) {
            out_load[k] = 0;
            for (int i : vis[k]) {
                const int wg = cls_lo(lo[i] + w[i], grid, ncls) - cls_lo(lo[i], grid, ncls);
                out_load[k] += it[i] / wg;
            }
        }
    return TMAC_HIP_OK;
}

// ---------------------------------------------------------------------------------------------
// Building a chain from noted calls: chain_build (at the end) runs the stages below in the order of their checks -- a recording that
// several stages would refuse is refused by the first.  analyse_flow .. plan_stream work on host data alone; commit_stream and commit
// create what lives on the device.
// ---------------------------------------------------------------------------------------------
// The A/B knobs of a build, read once per build, when one of these is constructed (tests set them between recordings).
static int env_int(const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}
struct BuildKnobs {
    int wpq = g_knobs.chain_wpq;                                      // tmac_hip_debug_chain_config: waves per row quad of every op (0: per-op choice)
    bool glu_epilogue = env_int("TMAC_CHAIN_GLU_EPILOGUE", 1) != 0;   // GLU in the producer where the recording allows it; 0 keeps the reader's form
    bool stream = env_int("TMAC_CHAIN_STREAM", 1) != 0;               // independent calls run in stream mode; 0 keeps k_decode_chain
    int ncls = env_int("TMAC_STREAM_NCLS", 16);                       // classes of the stream schedule, a power of two <= 16 and <= grid; 1: every range visits every op
    int visit_items = env_int("TMAC_STREAM_VISIT_ITEMS", 160);        // the schedule's `target` (sweep: profiles/r06_stream_schedule_sweep.txt)
    int qw = env_int("TMAC_STREAM_QW", -1);                           // -1: plan_stream's rule; 0 keeps the (quad x 64 units) form, 1 takes the quarter walk whenever the rows allow
    bool lpt = env_int("TMAC_STREAM_LPT", 1) != 0;                    // the schedule deals larger calls first; 0: in recorded order
    int split = env_int("TMAC_STREAM_SPLIT", 2);                      // workgroups per row range at most
    int split_bits = env_int("TMAC_STREAM_SPLIT_BITS", 3);            // the widest weights whose workgroups share a CU
    bool split_bits_set = getenv("TMAC_STREAM_SPLIT_BITS") != nullptr;   // (plan_stream lowers the default for recordings with a call of group size 64)
    int poll_sleep = env_int("TMAC_CHAIN_POLL_SLEEP", 8), poll_delay = env_int("TMAC_CHAIN_POLL_DELAY", 4);            // ChainArgs' fields of these names
    int issue_first = env_int("TMAC_CHAIN_ISSUE_FIRST", -1), poll_mode = env_int("TMAC_CHAIN_POLL_MODE", 0), poll_grid = env_int("TMAC_CHAIN_POLL_GRID", 0);
    explicit BuildKnobs(int grid) {
        ncls = std::min(std::max(ncls, 1), 16);
        while (ncls > grid || (ncls & (ncls - 1))) --ncls;
    }
};

// ---- data flow, on byte RANGES (ops run on workgroups that are not synchronised with each other; an op is ordered after another
// only through a hand-off: its activations are, transitively, made of the other's outputs) ----
struct Src { int op, mat; };                                  // output `mat` of call `op`; op -1: none, the vector comes from memory
struct ChainFlow {
    std::vector<Range> in_r;                                  // [op] the activations
    std::vector<std::vector<Range>> out_r;                    // [op][matrix] the outputs
    std::vector<Src> src, src2;                               // [op] where the activations / the second vector of a GLU come from
    std::vector<std::vector<char>> consumed, gathered;        // [op][matrix] the output is handed over inside the launch / through an exchange step
    std::vector<std::vector<char>> dep;                       // dep[k][i]: op k runs after op i has published everything
    std::vector<char> epi_of, glu_in_producer;                // [op] plan_glu_epilogue: the call publishes gate(gate) * up itself (1 + the gate: ChainOp::epi) / reads that product
};
// The most recent output before call i that overlaps r: the source of the vector call i reads at p, provided it IS that output.  Partial
// overlap with an earlier output cannot be handed over (the reader would see a mixture of launches): *partial is set, the caller refuses.
static Src latest_output(const std::vector<ChainRecOp>& rec, const ChainFlow& f, size_t i, const Range& r, const void* p, bool* partial) {
    *partial = false;
    for (size_t j = i; j-- > 0;)
        for (size_t m = 0; m < rec[j].C.size(); ++m)
            if (overlap(r, f.out_r[j][m])) { *partial = rec[j].C[m] != p; return Src{(int)j, (int)m}; }
    return Src{-1, -1};
}
static int32_t analyse_flow(const std::vector<ChainRecOp>& rec, const std::vector<ChainRecGather>& gat, tmac_dtype_t out, ChainFlow& f) {
    const size_t n = rec.size(), out_esz = out == TMAC_F16 ? 2 : 4;
    f.in_r.resize(n); f.out_r.resize(n);
    for (size_t i = 0; i < n; ++i) {
        f.in_r[i] = act_range(rec[i]);
        for (size_t m = 0; m < rec[i].w.size(); ++m) f.out_r[i].push_back(out_range(rec[i], m, out));
        for (size_t m = 0; m < f.out_r[i].size(); ++m)
            for (size_t m2 = 0; m2 < m; ++m2)
                if (overlap(f.out_r[i][m], f.out_r[i][m2])) return fail(TMAC_HIP_E_ARG, "op %zu: outputs %zu and %zu overlap", i, m2, m);
    }
    f.src.assign(n, Src{-1, -1}); f.src2.assign(n, Src{-1, -1});
    f.consumed.resize(n); f.gathered.resize(n);
    for (size_t i = 0; i < n; ++i) { f.consumed[i].assign(rec[i].w.size(), 0); f.gathered[i].assign(rec[i].w.size(), 0); }
    bool partial;
    for (size_t i = 0; i < n; ++i) {
        // activations that are the result of an exchange step recorded before this call: the latest such step decides; its
        // producer is the latest earlier call that writes the gathered buffer's send side
        const ChainRecGather* via = nullptr;
        for (const ChainRecGather& g : gat)
            if (g.pos <= i && g.recv == rec[i].B && (!via || g.pos >= via->pos)) via = &g;
        if (via) {
            for (size_t j = via->pos; j-- > 0 && f.src[i].op < 0;)
                for (size_t m = 0; m < rec[j].C.size(); ++m)
                    if (rec[j].C[m] == via->send) {
                        if (via->bytes != (size_t)rec[j].w[m]->s.Mw * out_esz)
                            return fail(TMAC_HIP_E_ARG, "op %zu: the exchange step gathers %zu bytes per rank, output %zu of op %zu has %zu", i, via->bytes, m, j,
                                        (size_t)rec[j].w[m]->s.Mw * out_esz);
                        if ((size_t)rec[i].w[0]->s.K > (size_t)via->world * rec[j].w[m]->s.Mw)
                            return fail(TMAC_HIP_E_ARG, "op %zu reads %d activations from a gather of %d x %d rows", i, rec[i].w[0]->s.K, via->world, rec[j].w[m]->s.Mw);
                        f.src[i] = Src{(int)j, (int)m};
                        f.consumed[j][m] = 1; f.gathered[j][m] = 1;
                        break;
                    }
            if (f.src[i].op < 0) return fail(TMAC_HIP_E_ARG, "op %zu reads a gathered buffer whose send side no earlier call of the chain writes", i);
            continue;
        }
        const Src s = latest_output(rec, f, i, f.in_r[i], rec[i].B, &partial);
        if (partial)
            return fail(TMAC_HIP_E_NOMATCH, "op %zu reads activations that overlap output %zu of op %zu without being that output: "
                                            "not representable as a hand-off", i, (size_t)s.mat, (size_t)s.op);
        if (s.op >= 0) { f.src[i] = s; f.consumed[s.op][s.mat] = 1; }
    }
    // the second vector of a GLU transform: the same rules as the activations (an earlier output, whole, or external memory)
    for (size_t i = 0; i < n; ++i) {
        if (!xf_has_glu(rec[i].xf)) continue;
        const Range r2{(const char*)rec[i].xf.in2, (const char*)rec[i].xf.in2 + (size_t)rec[i].w[0]->s.K * 2};
        const Src s = latest_output(rec, f, i, r2, rec[i].xf.in2, &partial);
        if (partial) return fail(TMAC_HIP_E_NOMATCH, "op %zu: the GLU's second vector overlaps output %zu of op %zu without being that output", i, (size_t)s.mat, (size_t)s.op);
        if (s.op >= 0) {
            if (f.gathered[s.op][s.mat]) return fail(TMAC_HIP_E_NOMATCH, "op %zu: a gathered output as the second vector of a GLU is not covered", i);
            f.src2[i] = s; f.consumed[s.op][s.mat] = 1;
        }
        if ((f.src2[i].op >= 0) != (f.src[i].op >= 0))
            return fail(TMAC_HIP_E_NOMATCH, "op %zu: the two vectors of a GLU must both be outputs of the chain or both be external", i);
    }
    // transitive closure over the hand-offs
    f.dep.assign(n, std::vector<char>(n, 0));
    for (size_t k = 0; k < n; ++k) {
        if (f.src[k].op >= 0) {
            f.dep[k] = f.dep[f.src[k].op];
            f.dep[k][f.src[k].op] = 1;
        }
        if (f.src2[k].op >= 0) {
            for (size_t q = 0; q < n; ++q) f.dep[k][q] |= f.dep[f.src2[k].op][q];
            f.dep[k][f.src2[k].op] = 1;
        }
    }
    return TMAC_HIP_OK;
}

// XfSpec -> ChainOp, the only two places that know the descriptor's spelling of a transform.  chain_epi: ChainOp::epi of the call that
// publishes gate(gate) * up for the reader with this transform -- 1 / 2 / 3 = silu / relu^2 / tanh-GELU.  fill_chain_xf: the reader's own
// fields as the kernel runs them (in_producer: the call in front publishes the product, so a GLU has nothing left to do and a GLU_NORM is
// a NORM of its handed-over `in`; otherwise the reader evaluates gate(in) * in2 itself, its gate in bits 8..9 of xf_flags; bit 1: the
// residual is the kept vector, bit 2: keep).  in2 is the layout's (an image or the caller's vector): describe_ops and commit.
static char chain_epi(const XfSpec& s) { return (char)(1 + s.gate); }
static void fill_chain_xf(ChainOp& o, const XfSpec& s, bool in_producer) {
    const bool norm = s.kind == TMAC_XF_NORM, glu_norm = s.kind == TMAC_XF_GLU_NORM;
    o.xf_kind = glu_norm ? TMAC_XF_NORM : (s.kind == TMAC_XF_GLU && in_producer) ? TMAC_XF_NONE : s.kind;
    if (o.xf_kind == TMAC_XF_GLU) o.xf_flags |= s.gate << 8;
    if (norm) {
        o.xf_flags |= (s.carry ? 2 : 0) | (s.keep ? 4 : 0);
        o.res = s.residual; o.res_out = s.residual_out;
    }
    if (norm || glu_norm) { o.gamma = s.gamma; memcpy(&o.eps_bits, &s.eps, 4); }
}

// GLU in the producer: when the two vectors of a GLU are outputs 0 and 1 of ONE earlier two-matrix call (gate and up) and nothing else
// in the chain reads the gate's hand-off image, the gate/up call publishes gate(gate) * up itself (the GLU's gate travels in epi_of) -- once per row, by the wave that
// publishes the rows anyway -- instead of all 256 workgroups of the reader evaluating K x (exp + rcp) each and polling two images
// (A/B: TMAC_CHAIN_GLU_EPILOGUE=0 keeps the reader's form).  Needs both quads of a row pair in one workgroup iteration: pairs are dealt.
// Fills f.epi_of / f.glu_in_producer; an up projection nobody else reads is no longer handed over (f.consumed).
static void plan_glu_epilogue(const std::vector<ChainRecOp>& rec, ChainFlow& f, int grid, const BuildKnobs& kn) {
    const size_t n = rec.size();
    f.epi_of.assign(n, 0); f.glu_in_producer.assign(n, 0);
    if (!kn.glu_epilogue) return;
    std::vector<std::vector<int>> readers(n);
    for (size_t j = 0; j < n; ++j) readers[j].assign(rec[j].w.size(), 0);
    for (size_t i = 0; i < n; ++i) {
        if (f.src[i].op >= 0) ++readers[f.src[i].op][f.src[i].mat];
        if (f.src2[i].op >= 0) ++readers[f.src2[i].op][f.src2[i].mat];
    }
    for (size_t i = 0; i < n; ++i) {
        if (!xf_has_glu(rec[i].xf) || f.src[i].op < 0 || f.src2[i].op != f.src[i].op || f.src[i].mat != 0 || f.src2[i].mat != 1) continue;
        const size_t j = (size_t)f.src[i].op;
        if (rec[j].w.size() != 2 || rec[j].w[0]->s.Mw != rec[j].w[1]->s.Mw || f.gathered[j][0] || f.gathered[j][1] || readers[j][0] != 1 || f.epi_of[j]) continue;
        const Shape& sj = rec[j].w[0]->s;
        const int nqj = 2 * sj.nquads(), nstj = (sj.K / 32 + 63) / 64;
        const int wq = kn.wpq ? kn.wpq : chain_pick_wpq(nqj, nstj, grid);
        if (CHAIN_NWV % wq || ((CHAIN_NWV / wq) & 1)) continue;          // pairs need an even number of quads per workgroup iteration
        f.epi_of[j] = chain_epi(rec[i].xf); f.glu_in_producer[i] = 1;
        if (readers[j][1] == 1) f.consumed[j][1] = 0;                    // nobody else reads the up projection through a hand-off
    }
}

// Where the hand-off images lie in the arena, as byte offsets: the descriptors get their pointers once, when the arena exists (commit).
constexpr size_t NO_IMAGE = ~(size_t)0;
struct ChainLayout {
    std::vector<std::array<size_t, 4>> gr;       // [op][matrix] this rank's rows in the image of a consumed output (ChainMat::GR); NO_IMAGE: nobody consumes it
    std::vector<size_t> in, in2;                 // [op] the image the op reads its activations / the second vector of its GLU from (ops that read one)
    int maxK = 0;
};

// The descriptors of k_decode_chain's ops; c holds the configuration (bits, zero points, dtypes, scale kind, grid, rank, world) and
// receives the ops, the arena's size and layout hash, the bytes of a launch and the LDS floats of the transforms.
static int32_t describe_ops(const std::vector<ChainRecOp>& rec, const ChainFlow& f, const BuildKnobs& kn, tmac_hip_chain& c, ChainLayout& lay) {
    const size_t n = rec.size();
    c.ops.resize(n);
    lay.gr.assign(n, {NO_IMAGE, NO_IMAGE, NO_IMAGE, NO_IMAGE});
    lay.in.assign(n, 0); lay.in2.assign(n, 0);
    for (size_t i = 0; i < n; ++i) {
        const ChainRecOp& r = rec[i];
        ChainOp& o = c.ops[i];
        memset(&o, 0, sizeof(o));
        const Shape& s0 = r.w[0]->s;
        const Src src = f.src[i], src2 = f.src2[i];
        if (r.act != TMAC_F16 && r.act != TMAC_F32) return fail(TMAC_HIP_E_NOMATCH, "op %zu: the decode chain takes fp16 or fp32 activations", i);
        if (r.act == TMAC_F32 && (src.op >= 0 || xf_has_glu(r.xf)))
            return fail(TMAC_HIP_E_NOMATCH, "op %zu: fp32 activations are covered for vectors in memory (an earlier output is handed over as fp16), without a GLU transform", i);
        if ((r.out == TMAC_F16) != (c.out_f16 != 0)) return fail(TMAC_HIP_E_NOMATCH, "op %zu: one output dtype per chain", i);
        if (s0.K > 8 * 3 * CHAIN_FT) return fail(TMAC_HIP_E_NOMATCH, "op %zu: K = %d beyond the decode chain's %d", i, s0.K, 8 * 3 * CHAIN_FT);
        if (((s0.m_groups >= 1) ? 2 : 0) != c.sm) return fail(TMAC_HIP_E_NOMATCH, "op %zu: per-group and unified scales cannot share a chain", i);
        if (r.perm && c.sm == 2) return fail(TMAC_HIP_E_NOMATCH, "op %zu: act-order handles are served with per-group scales only", i);
        int gu = 1;
        if (c.sm == 2) {
            if (s0.ags != s0.K || s0.K % 64 || s0.m_groups > CHAIN_US_MAX_GROUPS)
                return fail(TMAC_HIP_E_NOMATCH, "op %zu: the unified-scale chain covers one act group per row (act_group_size == K) and up to %d scales per matrix",
                            i, CHAIN_US_MAX_GROUPS);
        } else {
            gu = s0.gs / 32;
            if (s0.ags != 64 || s0.gs < 64 || (gu & (gu - 1)) || s0.K % s0.gs || s0.K % 64)
                return fail(TMAC_HIP_E_NOMATCH, "op %zu: the decode chain covers per-group scales (group >= 64, power of two) with act groups of 64", i);
            if (s0.gs == 64) c.g2 = 1;          // gu = 2, gs_shift = 1: a lane's two act groups of an item lie in two scale groups
        }
        int nq = 0;
        for (size_t m = 0; m < r.w.size(); ++m) {
            const tmac_hip_weights* w = r.w[m];
            const Shape& a = w->s;
            if (layout_of(a) != L_QUAD || !w->tiled_ok || w->fa) return fail(TMAC_HIP_E_NOMATCH, "op %zu matrix %zu is not registered in the QUAD layout", i, m);
            if (a.K != s0.K || a.bits != c.bits || a.gs != s0.gs || a.ags != s0.ags || a.zero_point != c.zp || a.m_groups != s0.m_groups ||
                (w->sc_dtype == F16) != (c.sc_f16 != 0))
                return fail(TMAC_HIP_E_ARG, "op %zu: the matrices of a chain share bits, zero points and scale dtype; those of an op also K and group size", i);
            if (c.sm == 2 && a.Mw % a.m_groups) return fail(TMAC_HIP_E_NOMATCH, "op %zu matrix %zu: rows not divisible by m_groups", i, m);
            nq += a.nquads();
            o.m[m].W = (const uint4*)w->W; o.m[m].SC = w->SC; o.m[m].C = r.C[m]; o.m[m].Mw = a.Mw; o.m[m].q_end = nq;
            if (f.consumed[i][m]) {
                if (r.out != TMAC_F16) return fail(TMAC_HIP_E_NOMATCH, "op %zu: outputs consumed inside the chain must be fp16", i);
                if (f.gathered[i][m] && a.Mw % 4) return fail(TMAC_HIP_E_NOMATCH, "op %zu: row shards of a gathered output must be whole row quads", i);
                // image of the output as its consumers see it: the rows of ALL ranks when it goes through an exchange step (rank r's
                // quads from r * nquads on)
                const size_t nq_img = (size_t)a.nquads() * (f.gathered[i][m] ? c.world : 1);
                const size_t my_off = f.gathered[i][m] ? (size_t)c.rank * a.nquads() * 16 : 0;
                lay.gr[i][m] = c.arena_bytes + my_off;
                c.layout_hash = (c.layout_hash ^ (nq_img * 16 + i * 4 + m)) * 1099511628211ull;
                c.arena_bytes += (nq_img * 16 + 255) & ~(size_t)255;
            }
            c.bytes += w->w_bytes + w->sc_bytes;
        }
        o.nmat = (int)r.w.size();
        for (int m = 0; m < 4; ++m) o.q_end[m] = (m < o.nmat - 1) ? o.m[m].q_end : 0x7fffffff;
        o.K = s0.K; o.nu = s0.K / 32; o.nst = (o.nu + 63) / 64; o.tstride = o.nst * 64 + 1;
        o.G = s0.K / 64; o.GP = o.nst * 32; o.nsg = c.sm == 2 ? 1 : s0.K / s0.gs;
        o.gs_shift = 0;
        for (int g = gu; g > 1; g >>= 1) ++o.gs_shift;
        o.m_groups = c.sm == 2 ? s0.m_groups : 0;
        o.total_q = nq;
        const int wpq = kn.wpq ? kn.wpq : chain_pick_wpq(nq, o.nst, c.grid);
        if (CHAIN_NWV % wpq) return fail(TMAC_HIP_E_ARG, "waves per quad must divide %d", CHAIN_NWV);
        set_wpq(o, wpq, CHAIN_NWV);
        if (nq / c.grid + 1 + o.ipi >= 4096) return fail(TMAC_HIP_E_NOMATCH, "op %zu: too many rows per workgroup for the decode chain", i);
        o.q_per = nq / c.grid; o.q_extra = nq % c.grid;
        if (f.epi_of[i]) { o.epi = f.epi_of[i]; c.xforms = 1; if (o.epi > 1) c.gates = 1; o.q_per = (nq / 2) / c.grid; o.q_extra = (nq / 2) % c.grid; }
        if (src.op >= 0) {
            const ChainMat& pm = c.ops[src.op].m[src.mat];
            const bool via_gather = f.gathered[src.op][src.mat] != 0;
            if (!via_gather && pm.Mw != o.K) return fail(TMAC_HIP_E_ARG, "op %zu reads an output of %d rows as %d activations", i, pm.Mw, o.K);
            // the image's first quad (a gathered image starts rank * nquads before this rank's part)
            const size_t my_off = via_gather ? (size_t)c.rank * ((pm.Mw + 3) / 4) * 16 : 0;
            lay.in[i] = lay.gr[src.op][src.mat] - my_off; o.in_gran = 1;
        } else {
            o.in = r.B; o.in_gran = 0;
            if (r.act == TMAC_F32) { o.in_gran = 2; c.xforms = 1;      // (the kernel instance with the extensions)
                if (chain_xf_region_floats(s0.K) > c.ext_floats) c.ext_floats = chain_xf_region_floats(s0.K); }
        }
        // ---- vector transform (tmac_hip_chain_xform; the field rules were applied when it was declared: tmac_xform.h)
        if (r.xf.kind != TMAC_XF_NONE) {
            const XfSpec& xf = r.xf;
            const int rf = chain_xf_region_floats(o.K);
            const bool reads_glu = xf.kind == TMAC_XF_GLU && !f.glu_in_producer[i];          // the reader evaluates gate(in) * in2 itself
            const bool runs = xf.kind != TMAC_XF_GLU || reads_glu;                           // (a GLU whose product the producer publishes leaves this op nothing to do)
            // GLU_NORM is served in the producer form only: the gate/up call publishes g = gate(gate) * up (fp16, like every handed-over
            // vector) and this call is a NORM of its handed-over `in` -- no residual, no carry -- which the kernel already runs
            if (xf.kind == TMAC_XF_GLU_NORM && !f.glu_in_producer[i])
                return fail(TMAC_HIP_E_NOMATCH, "op %zu: a GLU_NORM transform is recorded only where the call in front publishes silu(in) * in2 itself (in and in2 "
                                                "outputs 0 and 1 of one earlier two-matrix call that nothing else reads through a hand-off, not gathered, "
                                                "TMAC_CHAIN_GLU_EPILOGUE != 0, an even number of row quads per workgroup iteration): launch these calls one by one", i);
            if (runs) {
                c.xforms = 1;
                if (o.K > 2 * 8 * CHAIN_FT)
                    return fail(TMAC_HIP_E_NOMATCH, "op %zu: a %s transform is covered up to K = %d%s", i, xf.kind == TMAC_XF_NORM ? "NORM" : xf.kind == TMAC_XF_GLU ? "GLU" : "GLU_NORM",
                                2 * 8 * CHAIN_FT, xf.kind == TMAC_XF_GLU_NORM ? " (the NORM's limit)" : "");
            }
            if (xf.kind == TMAC_XF_NORM) {
                if (o.K > 8192 && (xf.keep || xf.carry)) return fail(TMAC_HIP_E_NOMATCH, "op %zu: a kept residual vector is covered up to K = 8192", i);
                if (xf.carry && c.carry_K != o.K) return fail(TMAC_HIP_E_ARG, "op %zu: no earlier NORM of the chain keeps a vector of %d values", i, o.K);
                if (xf.keep) { c.carry_K = o.K; if (rf > c.carry_floats) c.carry_floats = rf; }
            }
            if (runs && !xf.keep && rf > c.tmp_floats) c.tmp_floats = rf;
            if (xf.gamma && rf > c.gam_floats) c.gam_floats = rf;
            if (reads_glu) {
                if (xf.gate) c.gates = 1;
                if (src2.op >= 0) {
                    const ChainMat& p2 = c.ops[src2.op].m[src2.mat];
                    if (p2.Mw != o.K) return fail(TMAC_HIP_E_ARG, "op %zu: the GLU's second vector has %d rows, K = %d", i, p2.Mw, o.K);
                    lay.in2[i] = lay.gr[src2.op][src2.mat];
                } else o.in2 = xf.in2;
            }
            fill_chain_xf(o, xf, f.glu_in_producer[i] != 0);
        }
        // weight fragments per wave in front of the polls: ONE.  The poll then returns after a fabric round trip plus 24 KB per
        // CU, and the wait behind it does not hold the LUT build until all of the op's weights have landed.  Putting the whole
        // ring in front ("start the stream at once") measured slower even for the ops whose stream outlasts the hand-off:
        // llama-2-7B W2 0.764 -> 0.714 ms, W4 1.028 -> 0.983 ms per token (profiles/r03_chain_knobs.txt).
        o.in_gran |= 1 << 8;
        if (o.K > lay.maxK) lay.maxK = o.K;
    }
    return TMAC_HIP_OK;
}

// Hazards between ops that no hand-off orders.  Every workgroup reads an op's activations itself (each builds the whole
// LUT) and walks the ops in recorded order.  "Op j has published" therefore implies "every workgroup is past op i" for
// any i <= j only when every workgroup owns rows of op j (q_per >= 1).  A later op k may overwrite an EXTERNAL input of
// op i (a decoder's "next x = last output") exactly when such an op j lies between them on k's hand-off path.
// Inputs handed over inside the launch are read from the hand-off image, never from the user-visible buffer.
static int32_t check_hazards(const std::vector<ChainRecOp>& rec, const ChainFlow& f, const std::vector<ChainOp>& ops) {
    const size_t n = rec.size();
    auto all_past = [&](size_t i, size_t k) {
        for (size_t j = i; j < k; ++j)
            if (f.dep[k][j] && ops[j].q_per >= 1) return true;
        return false;
    };
    for (size_t k = 0; k < n; ++k)
        for (size_t m = 0; m < f.out_r[k].size(); ++m)
            for (size_t i = 0; i < k; ++i) {
                if (f.src[i].op < 0 && overlap(f.out_r[k][m], f.in_r[i]) && !all_past(i, k))
                    return fail(TMAC_HIP_E_NOMATCH, "op %zu overwrites activations that op %zu reads from memory and nothing in the chain orders the two "
                                                    "(no hand-off path from an op in which every workgroup owns rows): launch these calls one by one", k, i);
                for (size_t m2 = 0; m2 < f.out_r[i].size(); ++m2)
                    if (overlap(f.out_r[k][m], f.out_r[i][m2]) && !f.dep[k][i])
                        return fail(TMAC_HIP_E_NOMATCH, "ops %zu and %zu write overlapping outputs and nothing in the chain orders them", i, k);
            }
    // The vectors of the transforms take part in the same analysis: what a NORM / GLU reads from memory (residual, norm weights, an
    // external second vector) must not be written by the launch unless a hand-off orders the writer behind every reader; what a NORM
    // writes (residual_out: stored by the workgroups that own the index range, while the others may still be reading) must not be read
    // by the same or a later op of the launch (a later NORM takes it as TMAC_XF_CARRY), nor overlap any output.
    std::vector<std::vector<Range>> xf_rd(n);
    std::vector<Range> xf_wr(n, Range{nullptr, nullptr});
    for (size_t i = 0; i < n; ++i) {
        const XfSpec& xf = rec[i].xf;          // (fields the kind does not read are null)
        const size_t K = (size_t)rec[i].w[0]->s.K;
        if (xf.residual) xf_rd[i].push_back(Range{(const char*)xf.residual, (const char*)xf.residual + K * 4});
        if (xf.in2 && f.src2[i].op < 0) xf_rd[i].push_back(Range{(const char*)xf.in2, (const char*)xf.in2 + K * 2});
        if (xf.gamma) xf_rd[i].push_back(Range{(const char*)xf.gamma, (const char*)xf.gamma + K * 4});
        if (xf.residual_out) xf_wr[i] = Range{(const char*)xf.residual_out, (const char*)xf.residual_out + K * 4};
    }
    for (size_t k = 0; k < n; ++k) {
        for (size_t i = 0; i < n; ++i)
            for (const Range& r : xf_rd[i]) {
                for (size_t m = 0; m < f.out_r[k].size(); ++m)
                    if (overlap(f.out_r[k][m], r) && (i >= k || !all_past(i, k)))
                        return fail(TMAC_HIP_E_NOMATCH, "op %zu writes output %zu over a vector that the transform of op %zu reads from memory and nothing in the "
                                                        "chain orders the writer behind every reader", k, m, i);
                if (xf_wr[k].lo && overlap(xf_wr[k], r) && (i >= k || !all_past(i, k)))
                    return fail(TMAC_HIP_E_NOMATCH, "op %zu: residual_out overlaps a vector that the transform of op %zu reads from memory (a later NORM of the "
                                                    "launch takes the kept vector, TMAC_XF_CARRY)", k, i);
            }
        if (!xf_wr[k].lo) continue;
        for (size_t i = 0; i < n; ++i) {
            if (f.src[i].op < 0 && overlap(xf_wr[k], f.in_r[i]) && (i >= k || !all_past(i, k)))
                return fail(TMAC_HIP_E_NOMATCH, "op %zu: residual_out overlaps activations that op %zu reads from memory", k, i);
            for (size_t m = 0; m < f.out_r[i].size(); ++m)
                if (overlap(xf_wr[k], f.out_r[i][m])) return fail(TMAC_HIP_E_NOMATCH, "op %zu: residual_out overlaps output %zu of op %zu", k, m, i);
            if (i != k && xf_wr[i].lo && overlap(xf_wr[k], xf_wr[i])) return fail(TMAC_HIP_E_NOMATCH, "ops %zu and %zu: overlapping residual_out vectors", i, k);
        }
    }
    return TMAC_HIP_OK;
}

// ---- stream mode: nothing is handed over and nothing is transformed -- the calls are independent (SURVEY 8d's back-to-back GEMVs;
// a caller that evaluates many vectors against many matrices).  The reference's call structure then applies as it stands: tables
// once per activation vector (llama_cpp_init), lookups per matrix (llama_cpp_compute); see tmac_stream.hip.  The hazard analysis
// has already refused every write of the launch that touches a vector another op reads from memory.  TMAC_CHAIN_STREAM=0: A/B.
// The verdict (tmac_chain_indep.h) names the first call that stands in the way: a recording declared independent is refused with it.
static IndepVerdict independent(const std::vector<ChainRecOp>& rec, const std::vector<ChainRecGather>& gat, const ChainFlow& f) {
    std::vector<IndepOp> io(rec.size());
    for (size_t i = 0; i < rec.size(); ++i) io[i] = IndepOp{f.src[i].op, f.src2[i].op, (int)rec[i].xf.kind, f.epi_of[i]};
    return indep_verdict(io.data(), io.size(), gat.size());
}
static int32_t refuse_declared(const IndepVerdict& v) {
    static const char* const DECL = "the recording was declared independent (tmac_hip_chain_begin_independent)";
    switch (v.why) {
    case INDEP_FLOW: return fail(TMAC_HIP_E_ARG, "op %d reads an output of op %d as its activations: %s", v.op, v.other, DECL);
    case INDEP_FLOW2: return fail(TMAC_HIP_E_ARG, "op %d reads an output of op %d as the second vector of its GLU: %s", v.op, v.other, DECL);
    case INDEP_XFORM: return fail(TMAC_HIP_E_ARG, "op %d carries a vector transform: %s", v.op, DECL);
    case INDEP_EPILOGUE: return fail(TMAC_HIP_E_ARG, "op %d publishes a GLU's product for a later call: %s", v.op, DECL);
    default: return fail(TMAC_HIP_E_ARG, "an exchange step was recorded: %s", DECL);
    }
}
struct StreamPlan {
    std::vector<ChainOp> ops;             // the descriptors as k_lut_images / k_gemv_stream read them (img: written by commit_stream)
    std::vector<size_t> img_off;          // [op] byte offset of the op's LUT image among the images
    std::vector<int32_t> roles;           // the waves' role records, then the classes' visit counts
    size_t img_bytes = 0, lds_bytes = 0;
    int buf_u4 = 0, max_nst = 0, ncls = 1, vmax = 1, nsplit = 1;
    bool qw = true;
};
// The stream-mode form of independent ops (their k_decode_chain descriptors, by value), or nothing when that form does not fit: the
// recording then stays with k_decode_chain as described.
static std::optional<StreamPlan> plan_stream(std::vector<ChainOp> ops, int bits, bool g2, int grid, const BuildKnobs& kn) {
    StreamPlan p;
    p.ops = std::move(ops);
    const int nop = (int)p.ops.size(), ncls = p.ncls = kn.ncls;
    p.img_off.resize(nop);
    for (int i = 0; i < nop; ++i) {
        ChainOp& o = p.ops[i];
        o.img_u4 = stream_img_u4(o.K);
        p.img_off[i] = p.img_bytes;
        p.img_bytes += (size_t)o.img_u4 * 16;
        if (o.img_u4 > p.buf_u4) p.buf_u4 = o.img_u4;
        if (o.nst > p.max_nst) p.max_nst = o.nst;
        o.in_gran &= 2;                                               // (no fragments-in-front-of-the-polls count: there are no polls)
    }
    // ---- the schedule (tmac_chain.h, StreamArgs): which row ranges visit which op.  The per-visit costs of k_gemv_stream (two barriers,
    // the image, the waves' op change, waves without items in a short op: ~1.5 us per op whatever its size, profiles/r05_stream_knockouts.txt)
    // are paid per (workgroup, visit): an op that gives a row range fewer than `target` items is dealt to 1 / n of the ranges (n a power
    // of two) with n times the rows each, and the other classes of ranges work on other ops meanwhile.  Ops go to the least loaded aligned
    // block of classes, widest blocks and larger ops first (TMAC_STREAM_LPT=0: in recorded order; A/B); the cap on n that gives the shortest
    // modelled launch is taken (a lone call keeps all ranges).  TMAC_STREAM_NCLS=1: every range visits every op (the round-5 form; A/B).
    const int nwv = STREAM_NLW;
    // The quarter-walk form of the kernel (tmac_stream.hip, QW): rows dealt in groups of four quads, K walked in quarters of a 64-unit
    // step.  It saves the lookups a ragged last step wastes (K = 11008, 3200, 8640 ...) and is the faster form even without one
    // (profiles/r06_stream_qw.txt), so 1- and 2-bit recordings take it whenever every matrix has whole groups (rows % 16 == 0);
    // TMAC_STREAM_QW=0 keeps the (quad x 64 units) form, whose per-group-scale outputs are bit-identical to the stand-alone launches.
    {
        double it64 = 0, it16 = 0;
        for (const ChainOp& o : p.ops) {
            for (int m = 0; m < o.nmat; ++m) if (((o.m[m].Mw + 3) / 4) % 4) p.qw = false;
            it64 += (double)o.total_q * o.nst; it16 += (double)(o.total_q / 4) * ((o.nu + 15) / 16);
        }
        // 3- and 4-bit streams run at the memory system's rate already (6.1-6.4 TB/s), where four 256-byte pieces per wave-load cost more
        // than one KB: they take the form only when the ragged steps outweigh that, i.e. when it saves more than 15 % of the items
        // (it16 <= it64 always): W3 4096 x 11008 0.75 -> 0.65 with the form, W4 equal (profiles/r06_stream_qw.txt)
        if (kn.qw == 0 || (kn.qw < 0 && bits >= 3 && it16 > 0.85 * it64)) p.qw = false;
    }
    const bool qw = p.qw;
    auto op_q = [&](const ChainOp& o) { return qw ? o.total_q / 4 : o.total_q; };               // row units dealt: groups | quads
    auto op_nst = [&](const ChainOp& o) { return qw ? (o.nu + 15) / 16 : o.nst; };              // K steps walked: quarters | 64-unit steps
    std::vector<int> blk_lo, blk_w;
    std::vector<std::vector<int>> visits;
    {
        std::vector<double> items(nop);
        for (int i = 0; i < nop; ++i) items[i] = (double)op_q(p.ops[i]) * op_nst(p.ops[i]);
        stream_schedule(items, grid, ncls, kn.visit_items, kn.lpt, blk_lo, blk_w, visits);
    }
    for (int i = 0; i < nop; ++i) {
        ChainOp& o = p.ops[i];
        const int wlo = cls_lo(blk_lo[i], grid, ncls), wcnt = cls_lo(blk_lo[i] + blk_w[i], grid, ncls) - wlo;
        o.wg_lo = wlo;
        const int tq = op_q(o), nstw = op_nst(o);
        set_wpq(o, (!kn.wpq || nwv % o.wpq || o.wpq > nstw) ? chain_pick_wpq(tq, nstw, wcnt, nwv) : o.wpq, nwv);
        o.q_per = tq / wcnt; o.q_extra = tq % wcnt;
        if (tq / wcnt + 1 + o.ipi >= 4096) return std::nullopt;
        if (qw) for (int m = 0; m < 4; ++m) { if (o.q_end[m] != 0x7fffffff) o.q_end[m] /= 4; o.m[m].q_end /= 4; }      // the kernel counts groups
    }
    int vmax = 1;
    for (int k = 0; k < ncls; ++k) if ((int)visits[k].size() > vmax) vmax = (int)visits[k].size();
    p.vmax = vmax;
    // two workgroups per CU, alternate visits each (k_gemv_stream's nsplit): when both fit a CU's LDS.  TMAC_STREAM_SPLIT=1: A/B
    const size_t lds2 = stream_lds_bytes(p.buf_u4, (vmax + 1) / 2, qw);
    p.lds_bytes = stream_lds_bytes(p.buf_u4, vmax, qw);
    // Two workgroups are co-resident on a CU only with <= 64 VGPRs and <= 80 SGPRs each (measured, profiles/r05_stream_stamps.txt): 1- to
    // 3-bit weights fit with two fragments in flight per wave (3-bit: 4.06 -> 3.55 us on 4096 x 11008); 4-bit ones only with one,
    // which loses to one workgroup with two (5.15 against 4.68 us): they keep one workgroup per CU.  TMAC_STREAM_SPLIT_BITS: A/B.
    // G2 (a call of group size 64): a fragment carries a second scale word, and the 3-bit instance stays within 64 VGPRs only with ONE
    // fragment in flight -- the position 4-bit weights are in above, so such recordings keep one workgroup per CU as well (an explicit
    // TMAC_STREAM_SPLIT_BITS still decides: A/B)
    const int split_bits = (g2 && !kn.split_bits_set && kn.split_bits > 2) ? 2 : kn.split_bits;
    if (kn.split >= 2 && bits <= split_bits && vmax >= 2 && 2 * lds2 + 2048 <= 160 * 1024) { p.nsplit = 2; p.lds_bytes = lds2; }
    for (int ns = 3; ns <= kn.split && ns <= 4; ++ns) {            // (A/B builds with -DTMAC_STREAM_NLW=6: more, smaller workgroups per CU)
        const size_t ldsn = stream_lds_bytes(p.buf_u4, (vmax + ns - 1) / ns, qw);
        if (p.nsplit == ns - 1 && vmax >= ns && ns * (ldsn + 1024) <= 160 * 1024) { p.nsplit = ns; p.lds_bytes = ldsn; }
    }
    if (p.lds_bytes > 160 * 1024) return std::nullopt;
    // the waves' role records (tmac_chain.h) behind the images: one per (class, visit), then the classes' visit counts
    p.roles.assign((size_t)STREAM_ROLE_INTS * ncls * vmax + ncls, 0);
    for (int k = 0; k < ncls; ++k) {
        p.roles[(size_t)STREAM_ROLE_INTS * ncls * vmax + k] = (int32_t)visits[k].size();
        for (size_t v = 0; v < visits[k].size(); ++v) {
            const int i = visits[k][v];
            const ChainOp& o = p.ops[i];
            int32_t* r = p.roles.data() + ((size_t)k * vmax + v) * STREAM_ROLE_INTS;
            const int nstw = op_nst(o);
            r[SR_NST] = nstw; r[SR_IPI] = o.ipi; r[SR_NSG] = o.nsg; r[SR_GSH] = o.gs_shift; r[SR_NU] = o.nu;
            r[SR_QE0] = o.q_end[0]; r[SR_QE1] = o.q_end[1]; r[SR_QE2] = o.q_end[2];
            r[SR_QPER] = o.q_per; r[SR_QEXTRA] = o.q_extra;
            r[SR_IT_LO] = (o.q_per + o.ipi - 1) / o.ipi; r[SR_IT_HI] = (o.q_per + o.ipi) / o.ipi;
            r[SR_TSTRIDE] = o.tstride; r[SR_OP] = i; r[SR_WPQ] = o.wpq; r[SR_WLO] = o.wg_lo;
            for (int wl = 0; wl < STREAM_NLW; ++wl) {
                int32_t* rw = r + SR_COMMON + SRW_INTS * wl;
                const int qs = wl / o.wpq, h = wl - qs * o.wpq;
                auto nq = [&](int cnt) { return qs < cnt ? (cnt - 1 - qs) / o.ipi + 1 : 0; };
                rw[SRW_NQ] = nq(o.q_per) | (nq(o.q_per + 1) << 16);
                rw[SRW_NSTEPS] = h < nstw ? (nstw - h + o.wpq - 1) / o.wpq : 0;
                rw[SRW_H] = h; rw[SRW_QS] = qs;
            }
        }
    }
    return p;
}

// ---- what lives on the device ----
// a stream plan becomes the chain's form: its LUT images (zeroed) with the role records behind them, its descriptors
static int32_t commit_stream(tmac_hip_chain& c, StreamPlan& p) {
    const size_t role_bytes = p.roles.size() * sizeof(int32_t);
    if (hipMalloc(&c.images, p.img_bytes + role_bytes) != hipSuccess || hipMemset(c.images, 0, p.img_bytes) != hipSuccess ||
        hipMemcpy(static_cast<char*>(c.images) + p.img_bytes, p.roles.data(), role_bytes, hipMemcpyHostToDevice) != hipSuccess)
        return fail(TMAC_HIP_E_RUNTIME, "LUT image allocation failed (%zu bytes)", p.img_bytes + role_bytes);
    c.roles = reinterpret_cast<const int*>(static_cast<char*>(c.images) + p.img_bytes);
    c.nvis = c.roles + (size_t)STREAM_ROLE_INTS * p.ncls * p.vmax;
    c.ncls = p.ncls; c.vmax = p.vmax; c.qw = p.qw; c.nsplit = p.nsplit; c.max_nst = p.max_nst;
    c.ops = std::move(p.ops);
    for (size_t i = 0; i < c.ops.size(); ++i) c.ops[i].img = static_cast<const char*>(c.images) + p.img_off[i];
    c.stream = true; c.buf_u4 = p.buf_u4; c.lds_bytes = p.lds_bytes; c.xforms = 0;
    return TMAC_HIP_OK;
}
// k_decode_chain's LDS and residency (a chain that did not become a stream), the hand-off arena with the descriptors' pointers into
// it, the descriptors and the control word
static int32_t commit(tmac_hip_chain& c, const ChainLayout& lay) {
    if (!c.stream) {
        c.buf_u4 = chain_buf_u4(lay.maxK);
        c.lds_bytes = chain_lds_bytes(c.buf_u4, (int)c.ops.size(), c.carry_floats + c.tmp_floats + c.gam_floats + c.ext_floats);
        if (c.lds_bytes > 160 * 1024)
            return fail(TMAC_HIP_E_NOMATCH, "%zu calls with K up to %d need %zu bytes of LDS (LUT buffers + call descriptors): record shorter chains",
                        c.ops.size(), lay.maxK, c.lds_bytes);
        // one workgroup per CU must be resident at once: does the kernel fit a CU at all with this much LDS?
        ChainArgs probe;
        memset(&probe, 0, sizeof(probe));
        probe.nops = 1;
        int resident = 0;
        hipError_t e = launch_decode_chain(probe, c.bits, c.zp != 0, c.sc_f16 != 0, c.sm, c.g2 != 0, c.grid, c.lds_bytes, nullptr, &resident);
        if (e == hipErrorInvalidValue) return fail(TMAC_HIP_E_NOMATCH, "no decode-chain kernel for this configuration");
        if (e != hipSuccess || resident < 1)
            return fail(TMAC_HIP_E_NOMATCH, "the decode chain's workgroup does not fit a compute unit (%s, %zu bytes of LDS)",
                        e == hipSuccess ? "occupancy 0" : hipGetErrorString(e), c.lds_bytes);
    }
    if (c.arena_bytes) {
        // Peers write into this arena over xGMI while the local kernel polls it: fine-grained device memory (coherent across
        // devices inside a running kernel; coarse-grained allocations promise that at kernel boundaries only).  Single-GPU
        // chains keep the ordinary allocation.
        // Two halves, used by generation parity: a rank that has finished launch g may publish the first granules of launch g + 1
        // while a slower peer still polls the images of launch g (it cannot get further ahead: launch g + 1 needs the peer's rows).
        const hipError_t ea = c.world > 1 ? hipExtMallocWithFlags(&c.arena, 2 * c.arena_bytes, hipDeviceMallocFinegrained)
                                          : hipMalloc(&c.arena, 2 * c.arena_bytes);
        if (ea != hipSuccess || hipMemset(c.arena, 0, 2 * c.arena_bytes) != hipSuccess)
            return fail(TMAC_HIP_E_RUNTIME, "hand-off arena allocation failed (%zu bytes)", 2 * c.arena_bytes);
        char* const base = static_cast<char*>(c.arena);
        for (size_t i = 0; i < c.ops.size(); ++i) {
            ChainOp& o = c.ops[i];
            for (int m = 0; m < o.nmat; ++m)
                if (lay.gr[i][m] != NO_IMAGE) o.m[m].GR = reinterpret_cast<uint4*>(base + lay.gr[i][m]);
            if (o.in_gran & 1) o.in = base + lay.in[i];
            if ((o.in_gran & 1) && o.xf_kind == TMAC_XF_GLU) o.in2 = base + lay.in2[i];
        }
    }
    c.connected = c.world == 1;
    if (hipMalloc((void**)&c.d_ops, sizeof(ChainOp) * c.ops.size()) != hipSuccess ||
        hipMemcpy(c.d_ops, c.ops.data(), sizeof(ChainOp) * c.ops.size(), hipMemcpyHostToDevice) != hipSuccess)
        return fail(TMAC_HIP_E_RUNTIME, "descriptor upload failed");
    if (c.has_perm) {        // k_lut_images' second argument: one device permutation per op, null for the plain ones
        std::vector<const int32_t*> dp(c.ops.size(), nullptr);
        for (size_t i = 0; i < dp.size(); ++i) if (c.perms[i]) dp[i] = c.perms[i]->dev;
        if (hipMalloc((void**)&c.d_perms, sizeof(const int32_t*) * dp.size()) != hipSuccess ||
            hipMemcpy(c.d_perms, dp.data(), sizeof(const int32_t*) * dp.size(), hipMemcpyHostToDevice) != hipSuccess)
            return fail(TMAC_HIP_E_RUNTIME, "permutation table upload failed");
    }
    const unsigned ctl0[4] = {1u, 0u, 0u, 0u};
    if (hipMalloc((void**)&c.ctl, sizeof(ctl0)) != hipSuccess || hipMemcpy(c.ctl, ctl0, sizeof(ctl0), hipMemcpyHostToDevice) != hipSuccess)
        return fail(TMAC_HIP_E_RUNTIME, "control word allocation failed");
    // the granule fills above ran on the null stream; the chain is launched on the caller's (possibly non-blocking) stream
    if (hipStreamSynchronize(nullptr) != hipSuccess) return fail(TMAC_HIP_E_RUNTIME, "hand-off buffer initialisation failed");
    return TMAC_HIP_OK;
}

struct ChainFree { void operator()(tmac_hip_chain* c) const { (void)tmac_hip_chain_free(c); } };

int32_t tmac_host::chain_build(const std::vector<ChainRecOp>& rec, const std::vector<ChainRecGather>& gat, tmac_hip_chain** out, bool declared) {
    *out = nullptr;
    if (rec.empty()) return fail(TMAC_HIP_E_ARG, "nothing was recorded");
    int32_t rc = ensure_device();
    if (rc) return rc;
    int dev = 0, cus = 0;
    HIP_TRY(hipGetDevice(&dev));
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    if (cus < 1) return fail(TMAC_HIP_E_RUNTIME, "no compute units reported");
    std::unique_ptr<tmac_hip_chain, ChainFree> c(new tmac_hip_chain());      // (freed on every refusal below)
    c->grid = (g_knobs.chain_grid > 0 && g_knobs.chain_grid < cus) ? g_knobs.chain_grid : cus;   // one workgroup per CU; residency is checked by commit
    const BuildKnobs kn(c->grid);
    for (const ChainRecGather& g : gat) {
        if (g.world != gat[0].world || g.rank != gat[0].rank) return fail(TMAC_HIP_E_ARG, "the exchange steps of a chain share rank and world size");
        c->rank = g.rank; c->world = g.world;
    }
    const tmac_hip_weights* w0 = rec[0].w[0];
    c->bits = w0->s.bits; c->zp = w0->s.zero_point; c->sc_f16 = w0->sc_dtype == F16; c->out_f16 = rec[0].out == TMAC_F16;
    c->sm = (w0->s.m_groups >= 1) ? 2 : 0;
    if (c->bits < 1 || c->bits > 4) return fail(TMAC_HIP_E_NOMATCH, "the decode chain is built for 1- to 4-bit weights");

    ChainFlow flow;
    if ((rc = analyse_flow(rec, gat, rec[0].out, flow)) != TMAC_HIP_OK) return rc;
    plan_glu_epilogue(rec, flow, c->grid, kn);
    const IndepVerdict indep = independent(rec, gat, flow);
    // a declared-independent recording becomes a stream or nothing: refused here, by the first call that breaks the declaration, before
    // anything is said about k_decode_chain's own limits
    if (declared && indep.why != INDEP_OK) return refuse_declared(indep);
    for (const ChainRecOp& r : rec) {
        if (r.perm && !declared) return fail(TMAC_HIP_E_ARG, "a call on act-order handles is recorded only in a recording declared independent");
        c->has_perm = c->has_perm || r.perm;
    }
    ChainLayout lay;
    if ((rc = describe_ops(rec, flow, kn, *c, lay)) != TMAC_HIP_OK) return rc;
    if ((rc = check_hazards(rec, flow, c->ops)) != TMAC_HIP_OK) return rc;
    std::optional<StreamPlan> plan;
    if (kn.stream && indep.why == INDEP_OK) plan = plan_stream(c->ops, c->bits, c->g2 != 0, c->grid, kn);
    if (declared && !plan)
        return fail(TMAC_HIP_E_ARG, kn.stream ? "the stream planner has no form for these calls (rows per workgroup, or LDS for the LUT images): the recording was declared independent "
                                                "(tmac_hip_chain_begin_independent) and is not built as k_decode_chain"
                                              : "TMAC_CHAIN_STREAM=0 keeps every recording out of stream mode: the recording was declared independent "
                                                "(tmac_hip_chain_begin_independent) and is not built as k_decode_chain");
    if (c->has_perm)         // (the chain owns its ops' permutations: the device arrays outlive the handles and the caller's objects)
        for (const ChainRecOp& r : rec) c->perms.push_back(r.perm);
    if (plan && (rc = commit_stream(*c, *plan)) != TMAC_HIP_OK) return rc;
    if ((rc = commit(*c, lay)) != TMAC_HIP_OK) return rc;
    // A workgroup reaches the polls of an op right after publishing its own share of the previous one: the first poll cannot
    // succeed before the slowest producer's stores have crossed the fabric (~1 us), and every failed poll is 16 KB per workgroup
    // of fabric traffic that the stores compete with.  Waiting ~0.75 us before the first poll and ~0.5 us between polls:
    // 0.757 -> 0.735 ms per llama-2-7B token (profiles/r02_chain_prefetch_ab.txt, E).
    c->poll_sleep = kn.poll_sleep; c->poll_delay = kn.poll_delay; c->issue_first = kn.issue_first; c->poll_mode = kn.poll_mode; c->poll_grid = kn.poll_grid;
    *out = c.release();
    return TMAC_HIP_OK;
}

extern "C" int32_t tmac_hip_debug_chain_grid(int workgroups) {
    if (workgroups < 0) return fail(TMAC_HIP_E_ARG, "negative grid");
    g_knobs.chain_grid = workgroups;
    return TMAC_HIP_OK;
}

extern "C" int32_t tmac_hip_debug_chain_config(int force_wpq, unsigned spin_limit) {
    if (force_wpq < 0 || (force_wpq && CHAIN_NWV % force_wpq)) return fail(TMAC_HIP_E_ARG, "waves per quad must divide %d", CHAIN_NWV);
    g_knobs.chain_wpq = force_wpq;
    if (spin_limit) g_knobs.chain_spin_limit = spin_limit;
    return TMAC_HIP_OK;
}
