// tmac_tuner.cpp — launch-configuration tuner of the fused decode kernel.
#include "tmac_host.h"

using namespace tmac_host;

// ---------------------------------------------------------------------------------------------
// launch-configuration tuner (what autotvm's grid search over (bm, kfactor, bn) is to the reference's
// CPU kernels, python/t_mac/ops/base.py:84-127 + qgemm.py:98-116, the search over (threads per workgroup, waves per row
// quad) is to k_gemv_quad).  Measured once per (bits, K, row quads, matrices, quantisation flavour) on the device, kept in
// a table that the fused entry point consults before its built-in heuristic, and persisted as a small text file.
// ---------------------------------------------------------------------------------------------
struct TuneKey {
    int bits, K, total_q, nmat, flavour;   // flavour: zero_point | m_groups>=1 << 1 | fp16 scales << 2 | fp16 acts << 3
    bool operator<(const TuneKey& o) const {
        if (bits != o.bits) return bits < o.bits;
        if (K != o.K) return K < o.K;
        if (total_q != o.total_q) return total_q < o.total_q;
        if (nmat != o.nmat) return nmat < o.nmat;
        return flavour < o.flavour;
    }
};
struct TuneVal { int ft, wpq; float us; };
static std::map<TuneKey, TuneVal> g_tuned;
static std::mutex g_tune_mu;
static bool g_tune_env_loaded = false;

static TuneKey tune_key(const FusedArgs& fa, int total_q) {
    TuneKey k;
    k.bits = fa.s.bits; k.K = fa.s.K; k.total_q = total_q; k.nmat = fa.nmat;
    k.flavour = (fa.s.zero_point ? 1 : 0) | (fa.s.m_groups >= 1 ? 2 : 0) | (fa.sc_f16 ? 4 : 0) | (fa.act_f16 ? 8 : 0);
    return k;
}

extern "C" int32_t tmac_hip_tune_load(const char* path) {
    if (!path) return fail(TMAC_HIP_E_ARG, "null path");
    std::ifstream f(path);
    if (!f) return fail(TMAC_HIP_E_ARG, "cannot open tuning file %s", path);
    std::string line;
    int n = 0;
    std::lock_guard<std::mutex> lk(g_tune_mu);
    while (std::getline(f, line)) {
        if (line.empty() || line[0] == '#') continue;
        TuneKey k; TuneVal v;
        if (sscanf(line.c_str(), "%d %d %d %d %d %d %d %f", &k.bits, &k.K, &k.total_q, &k.nmat, &k.flavour, &v.ft, &v.wpq, &v.us) != 8)
            return fail(TMAC_HIP_E_ARG, "%s: malformed line '%s'", path, line.c_str());
        const bool ok = (v.ft == 512 && (v.wpq == 1 || v.wpq == 2)) || (v.ft == 768 && v.wpq >= 1 && v.wpq <= 3) ||
                        (v.ft == 1024 && (v.wpq == 1 || v.wpq == 2 || v.wpq == 4));
        if (!ok) return fail(TMAC_HIP_E_ARG, "%s: (%d, %d) is not a launch configuration of k_gemv_quad", path, v.ft, v.wpq);
        g_tuned[k] = v;
        ++n;
    }
    return n;
}

extern "C" int32_t tmac_hip_tune_save(const char* path) {
    if (!path) return fail(TMAC_HIP_E_ARG, "null path");
    std::ofstream f(path);
    if (!f) return fail(TMAC_HIP_E_ARG, "cannot write tuning file %s", path);
    std::lock_guard<std::mutex> lk(g_tune_mu);
    f << "# libtmac_hip k_gemv_quad launch configurations: bits K row_quads matrices flavour | threads waves_per_quad us\n";
    for (const auto& kv : g_tuned) {
        char buf[160];
        snprintf(buf, sizeof(buf), "%d %d %d %d %d %d %d %.3f\n", kv.first.bits, kv.first.K, kv.first.total_q, kv.first.nmat,
                 kv.first.flavour, kv.second.ft, kv.second.wpq, kv.second.us);
        f << buf;
    }
    return (int32_t)g_tuned.size();
}

extern "C" int32_t tmac_hip_tune_clear(void) {
    std::lock_guard<std::mutex> lk(g_tune_mu);
    g_tuned.clear();
    return TMAC_HIP_OK;
}

void tmac_host::tuned_config(const FusedArgs& fa, int total_q, int& ft, int& wpq) {
    bool load_env = false;
    {
        std::lock_guard<std::mutex> lk(g_tune_mu);
        load_env = !g_tune_env_loaded;
        g_tune_env_loaded = true;
    }
    if (load_env)   // $TMAC_HIP_TUNE_FILE: a table saved by an earlier run, picked up on first use
        if (const char* e = getenv("TMAC_HIP_TUNE_FILE")) (void)tmac_hip_tune_load(e);
    std::lock_guard<std::mutex> lk(g_tune_mu);
    auto it = g_tuned.find(tune_key(fa, total_q));
    if (it != g_tuned.end()) { ft = it->second.ft; wpq = it->second.wpq; }
}
// Times every launch configuration of k_gemv_quad on the given matrices (decode, N = 1) and records the fastest.
// The weights are replicated until the copies exceed the 256 MB MALL several times over and the timed graph walks the
// copies round-robin, so that every launch streams its weights from HBM as it does inside a model.
extern "C" int32_t tmac_hip_autotune_fused(const tmac_hip_weights* const* wl, int nmat, tmac_dtype_t act_dtype,
                                           tmac_dtype_t out_dtype, int* best_ft, int* best_wpq, float* best_us,
                                           float* heuristic_us) {
    if (!wl || nmat < 1 || nmat > 4) return fail(TMAC_HIP_E_ARG, "bad autotune arguments (1..4 matrices)");
    int32_t rc = ensure_device();
    if (rc) return rc;
    if ((rc = defer_barrier())) return rc;    // (the timed launches are not queued; what the thread has queued goes first)
    size_t bytes = 0;
    for (int i = 0; i < nmat; ++i) {
        if (!wl[i] || layout_of(wl[i]->s) != L_QUAD || !wl[i]->tiled_ok) return fail(TMAC_HIP_E_NOMATCH, "matrix %d is not registered in the QUAD layout", i);
        bytes += wl[i]->w_bytes + wl[i]->sc_bytes;
    }
    int R = (int)(((size_t)768 << 20) / (bytes ? bytes : 1)) + 1;
    if (R < 2) R = 2;
    if (R > 192) R = 192;
    std::vector<void*> allocs;
    auto release = [&]() { for (void* p : allocs) (void)hipFree(p); allocs.clear(); };
    auto dalloc = [&](size_t n) -> void* { void* p = nullptr; if (hipMalloc(&p, n) != hipSuccess) return nullptr; allocs.push_back(p); return p; };
    hipStream_t st = nullptr;
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) return fail(TMAC_HIP_E_RUNTIME, "stream create failed");
    const Shape& s0 = wl[0]->s;
    void* Bd = dalloc((size_t)s0.K * 4);
    std::vector<char*> Wc(nmat), Sc(nmat);
    std::vector<void*> Cd(nmat);
    bool ok = Bd != nullptr;
    for (int i = 0; i < nmat && ok; ++i) {
        Wc[i] = (char*)dalloc(wl[i]->w_bytes * R);
        Sc[i] = (char*)dalloc(wl[i]->sc_bytes * R);
        Cd[i] = dalloc((size_t)wl[i]->s.Mw * 4);
        ok = Wc[i] && Sc[i] && Cd[i];
        for (int r = 0; r < R && ok; ++r)
            ok = hipMemcpyAsync(Wc[i] + (size_t)r * wl[i]->w_bytes, wl[i]->W, wl[i]->w_bytes, hipMemcpyDeviceToDevice, st) == hipSuccess &&
                 hipMemcpyAsync(Sc[i] + (size_t)r * wl[i]->sc_bytes, wl[i]->SC, wl[i]->sc_bytes, hipMemcpyDeviceToDevice, st) == hipSuccess;
    }
    // activations: a fixed non-trivial pattern (0x3c3c... is 1.06 in fp16, 0.0115 in fp32); timing does not depend on values
    ok = ok && hipMemsetAsync(Bd, 0x3c, (size_t)s0.K * 4, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
    if (!ok) { release(); (void)hipStreamDestroy(st); return fail(TMAC_HIP_E_RUNTIME, "autotune: device allocation / copy failed"); }

    // the call on the scratch vectors, its matrices replaced by replica r (the MFMA accumulate whatever the variant knob says)
    const FusedCall call{wl, nmat, Bd, act_dtype, Cd.data(), out_dtype, 1, st};
    int total_q = 0;
    auto make_args = [&](int r) {
        FusedArgs fa;
        total_q = fill_fused_args(fa, call);
        for (int i = 0; i < nmat; ++i) {
            fa.m[i].W = (const uint4*)(Wc[i] + (size_t)r * wl[i]->w_bytes);
            fa.m[i].SC = Sc[i] + (size_t)r * wl[i]->sc_bytes;
        }
        fa.acc_mfma = 1;
        return fa;
    };
    auto time_config = [&](int ft, int wpq, float& us) -> hipError_t {
        hipError_t e = launch_gemv_quad(make_args(0), 1, true, ft, wpq, false, st);   // validity probe + code-object warm-up
        if (e != hipSuccess) return e;
        if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
        hipGraph_t g = nullptr; hipGraphExec_t ge = nullptr;
        if ((e = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal)) != hipSuccess) return e;
        for (int r = 0; r < R && e == hipSuccess; ++r) e = launch_gemv_quad(make_args(r), 1, true, ft, wpq, false, st);
        hipError_t e2 = hipStreamEndCapture(st, &g);
        if (e == hipSuccess) e = e2;
        if (e == hipSuccess) e = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
        hipEvent_t t0 = nullptr, t1 = nullptr;
        if (e == hipSuccess) e = hipEventCreate(&t0);
        if (e == hipSuccess) e = hipEventCreate(&t1);
        float best = 1e30f;
        for (int rep = 0; rep < 6 && e == hipSuccess; ++rep) {   // first replay warms up; best of the rest
            if ((e = hipEventRecord(t0, st)) != hipSuccess) break;
            if ((e = hipGraphLaunch(ge, st)) != hipSuccess) break;
            if ((e = hipEventRecord(t1, st)) != hipSuccess) break;
            if ((e = hipEventSynchronize(t1)) != hipSuccess) break;
            float ms = 0.f;
            if ((e = hipEventElapsedTime(&ms, t0, t1)) != hipSuccess) break;
            if (rep > 0 && ms < best) best = ms;
        }
        if (t0) (void)hipEventDestroy(t0);
        if (t1) (void)hipEventDestroy(t1);
        if (ge) (void)hipGraphExecDestroy(ge);
        if (g) (void)hipGraphDestroy(g);
        us = best * 1000.f / R;
        return e;
    };
    static const int cand[][2] = {{0, 0}, {512, 1}, {512, 2}, {768, 1}, {768, 2}, {768, 3}, {1024, 1}, {1024, 2}, {1024, 4}};
    TuneVal bestv{0, 0, 1e30f};
    float heur = 0.f;
    hipError_t err = hipSuccess;
    for (const auto& c : cand) {
        float us = 0.f;
        hipError_t e = time_config(c[0], c[1], us);
        if (e == hipErrorInvalidValue) { (void)hipGetLastError(); continue; }   // configuration not offered for this shape
        if (e != hipSuccess) { err = e; break; }
        if (c[0] == 0) { heur = us; continue; }
        if (us < bestv.us) bestv = TuneVal{c[0], c[1], us};
    }
    release();
    (void)hipStreamDestroy(st);
    if (err != hipSuccess) return fail(TMAC_HIP_E_RUNTIME, "autotune: %s", hipGetErrorString(err));
    if (bestv.ft == 0) return fail(TMAC_HIP_E_NOMATCH, "no k_gemv_quad configuration for these matrices");
    // the heuristic's choice stands unless a candidate beats it by more than the run-to-run noise of the measurement
    if (heur > 0.f && bestv.us > 0.96f * heur) {
        bestv.us = heur;
        bestv.ft = 0;
    }
    if (bestv.ft) {
        const FusedArgs fa = make_args(0);
        std::lock_guard<std::mutex> lk(g_tune_mu);
        g_tuned[tune_key(fa, total_q)] = bestv;
    }
    if (best_ft) *best_ft = bestv.ft;
    if (best_wpq) *best_wpq = bestv.ft ? bestv.wpq : 0;
    if (best_us) *best_us = bestv.us;
    if (heuristic_us) *heuristic_us = heur;
    return TMAC_HIP_OK;
}
