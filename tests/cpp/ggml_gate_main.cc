// One BitNet-b1.58-2B-4T-shaped layer through the ggml glue (include/ggml-tmac-hip.h), twice: as ONE recorded segment with
// ffn_sub_norm(relu(gate)^2 * up) declared by ggml_tmac_hip_segment_glu_gate(up, TMAC_XF_GATE_RELU2, w, eps), and call by call with
// ggml_tmac_hip_mul_mat_dev_xf(kind 4 | TMAC_XF_GATE_RELU2 = 0x104) in front of the down projection.  Every tensor of both passes is dumped
// (seg_* / cbc_*); tests/test_gpu_ggml_gate.py recomputes each stage with the oracle.
// usage: ggml_gate_main <dir> H F bits      (dir: kcfg.ini, blob_<name>.bin, h0.bin, g1.bin, g2.bin (fp32 [H]), g3.bin (fp32 [F]), attn.bin (fp16 [H]))
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "ggml-tmac-hip.h"
#include "tmac_hip.h"      // TMAC_XF_GLU_NORM, TMAC_XF_GATE_*

extern "C" int hipMalloc(void**, size_t);
extern "C" int hipMemcpy(void*, const void*, size_t, int);
extern "C" int hipMemcpyAsync(void*, const void*, size_t, int, void*);
extern "C" int hipMemset(void*, int, size_t);

static std::vector<char> slurp(const std::string& p) {
    std::ifstream f(p, std::ios::binary);
    return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}
static void* dev(const std::vector<char>& h) {
    void* d = nullptr;
    if (hipMalloc(&d, h.size()) || hipMemcpy(d, h.data(), h.size(), 1)) { fprintf(stderr, "device upload failed\n"); exit(7); }
    return d;
}
static void* dzero(size_t n) {
    void* d = nullptr;
    if (hipMalloc(&d, n) || hipMemset(d, 0, n)) { fprintf(stderr, "device allocation failed\n"); exit(7); }
    return d;
}
static void dump(const std::string& p, const void* d, size_t n) {
    std::vector<char> h(n);
    if (hipMemcpy(h.data(), d, n, 2)) { fprintf(stderr, "download failed\n"); exit(8); }
    std::ofstream(p, std::ios::binary).write(h.data(), (std::streamsize)n);
}
#define CK(x) do { if ((x)) { fprintf(stderr, "%s: %s\n", #x, ggml_tmac_hip_last_error()); return 6; } } while (0)

int main(int argc, char** argv) {
    if (argc < 5) return 2;
    const std::string d = argv[1];
    const int H = atoi(argv[2]), F = atoi(argv[3]), bits = atoi(argv[4]);
    if (ggml_tmac_hip_init((d + "/kcfg.ini").c_str(), 0)) { fprintf(stderr, "init: %s\n", ggml_tmac_hip_last_error()); return 3; }
    const char* names[7] = {"q", "k", "v", "o", "gate", "up", "down"};
    const int rows[7] = {H, H, H, H, F, F, H}, cols[7] = {H, H, H, H, H, H, F};
    std::vector<std::vector<char>> blobs(7);
    tmac_ggml_tensor w[7];
    for (int m = 0; m < 7; ++m) {
        blobs[m] = slurp(d + "/blob_" + names[m] + ".bin");
        w[m] = tmac_ggml_tensor{{cols[m], rows[m], 1, 1}, blobs[m].data(), nullptr};
        if (!ggml_tmac_hip_can_mul_mat(&w[m], bits)) { fprintf(stderr, "no kcfg entry for %s\n", names[m]); return 4; }
        CK(ggml_tmac_hip_upload(&w[m], bits));
    }
    float* h0 = (float*)dev(slurp(d + "/h0.bin"));
    float *g1 = (float*)dev(slurp(d + "/g1.bin")), *g2 = (float*)dev(slurp(d + "/g2.bin")), *g3 = (float*)dev(slurp(d + "/g3.bin"));
    void* attn = dev(slurp(d + "/attn.bin"));
    const tmac_ggml_tensor *wqkv[3] = {&w[0], &w[1], &w[2]}, *wo[1] = {&w[3]}, *wgu[2] = {&w[4], &w[5]}, *wd[1] = {&w[6]};
    for (int pass = 0; pass < 2; ++pass) {
        const std::string tag = pass == 0 ? "/seg_" : "/cbc_";
        float *t2 = (float*)dzero(sizeof(float) * H), *t3 = (float*)dzero(sizeof(float) * H);
        void *qkv[3], *o = dzero(2 * (size_t)H), *gu[2] = {dzero(2 * (size_t)F), dzero(2 * (size_t)F)}, *dn = dzero(2 * (size_t)H);
        for (int k = 0; k < 3; ++k) qkv[k] = dzero(2 * (size_t)H);
        if (pass == 0) {
            // one recorded segment: o -> [+ h0, RMSNorm; t kept] -> gate/up -> [RMSNorm(relu(gate)^2 * up)] -> down -> [+ kept t, RMSNorm] -> q/k/v
            ggml_tmac_hip_segment* seg = nullptr;
            // a gate that is none of the three is refused where it is declared, and declares nothing: the recording goes on without it
            CK(ggml_tmac_hip_segment_begin());
            if (ggml_tmac_hip_segment_glu_gate(gu[1], 0x300, g3, 1e-5f) == 0) { fprintf(stderr, "gate 0x300 accepted\n"); return 10; }
            if (ggml_tmac_hip_segment_glu_gate(gu[1], 1, nullptr, 0.0f) == 0) { fprintf(stderr, "gate 1 (no TMAC_XF_GATE_* value) accepted\n"); return 10; }
            CK(ggml_tmac_hip_segment_mul_mat(wo, 1, attn, &o));
            CK(ggml_tmac_hip_segment_norm(h0, 0, g2, 1e-5f, nullptr, 1));
            CK(ggml_tmac_hip_segment_mul_mat(wgu, 2, o, gu));
            CK(ggml_tmac_hip_segment_glu_gate(gu[1], TMAC_XF_GATE_RELU2, g3, 1e-5f));
            CK(ggml_tmac_hip_segment_mul_mat(wd, 1, gu[0], &dn));
            CK(ggml_tmac_hip_segment_norm(nullptr, 1, g1, 1e-5f, t3, 0));
            CK(ggml_tmac_hip_segment_mul_mat(wqkv, 3, dn, qkv));
            CK(ggml_tmac_hip_segment_end(&seg));
            for (int tok = 0; tok < 2; ++tok) {      // the second token replays the recording
                CK(ggml_tmac_hip_segment_compute(seg));
                CK(ggml_tmac_hip_segment_wait(seg));
            }
            ggml_tmac_hip_segment_free(seg);
        } else {
            // the same calls one by one: what a caller issues when _end refuses the recording; the residual stream in buffers of its own
            CK(ggml_tmac_hip_mul_mat_dev(wo, 1, attn, 0, &o, 0));
            CK(ggml_tmac_hip_mul_mat_dev_xf(wgu, 2, o, 0, 1, nullptr, h0, g2, 1e-5f, t2, gu, 0));
            CK(ggml_tmac_hip_mul_mat_dev_xf(wd, 1, gu[0], 0, TMAC_XF_GLU_NORM | TMAC_XF_GATE_RELU2, gu[1], nullptr, g3, 1e-5f, nullptr, &dn, 0));
            CK(ggml_tmac_hip_mul_mat_dev_xf(wqkv, 3, dn, 0, 1, nullptr, t2, g1, 1e-5f, t3, qkv, 0));
            CK(ggml_tmac_hip_synchronize());
            // refusals reach the caller (and leave dn as the valid call wrote it): the sub-layer norm takes no residual, the gate is one of three, a norm takes none
            if (ggml_tmac_hip_mul_mat_dev_xf(wd, 1, gu[0], 0, 0x104, gu[1], t2, g3, 1e-5f, nullptr, &dn, 0) == 0) { fprintf(stderr, "kind 0x104 with a residual accepted\n"); return 10; }
            if (ggml_tmac_hip_mul_mat_dev_xf(wd, 1, gu[0], 0, 4 | 0x300, gu[1], nullptr, g3, 1e-5f, nullptr, &dn, 0) == 0) { fprintf(stderr, "gate 0x300 accepted\n"); return 10; }
            if (ggml_tmac_hip_mul_mat_dev_xf(wd, 1, gu[0], 0, 1 | 0x100, nullptr, nullptr, g3, 1e-5f, nullptr, &dn, 0) == 0) { fprintf(stderr, "a gate on a norm accepted\n"); return 10; }
            CK(ggml_tmac_hip_synchronize());
        }
        dump(d + tag + "t3.bin", t3, sizeof(float) * H);
        for (int k = 0; k < 3; ++k) dump(d + tag + names[k] + ".bin", qkv[k], 2 * (size_t)H);
        dump(d + tag + "o.bin", o, 2 * (size_t)H);
        dump(d + tag + "gate.bin", gu[0], 2 * (size_t)F);
        dump(d + tag + "up.bin", gu[1], 2 * (size_t)F);
        dump(d + tag + "down.bin", dn, 2 * (size_t)H);
    }
    for (int m = 0; m < 7; ++m) ggml_tmac_hip_free(&w[m]);
    printf("RESULT ok\n");
    return 0;
}
