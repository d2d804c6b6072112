// The ggml glue's transformed mat-muls for several rows (include/ggml-tmac-hip.h: ggml_tmac_hip_mul_mat_dev_xf_rows): the MLP half of a
// llama-shaped layer for N rows at once -- gate/up behind [+ residual, RMSNorm], down behind [silu(gate) * up] -- with the element-wise
// operators inside the LUT builds.  Every tensor is dumped; tests/test_gpu_ggml_xf_rows.py recomputes each stage with the oracle.
// usage: ggml_xf_rows_main <dir> H F bits N     (dir: kcfg.ini, blob_<name>.bin, x.bin (fp16 [N][H]), h.bin (fp32 [N][H]), g.bin (fp32 [H]))
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "ggml-tmac-hip.h"

extern "C" int hipMalloc(void**, size_t);
extern "C" int hipMemcpy(void*, const void*, size_t, int);
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
    if (argc < 6) return 2;
    const std::string d = argv[1];
    const int H = atoi(argv[2]), F = atoi(argv[3]), bits = atoi(argv[4]), N = atoi(argv[5]);
    if (ggml_tmac_hip_init((d + "/kcfg.ini").c_str(), 0)) { fprintf(stderr, "init: %s\n", ggml_tmac_hip_last_error()); return 3; }
    const char* names[3] = {"gate", "up", "down"};
    const int rows[3] = {F, F, H}, cols[3] = {H, H, F};
    std::vector<std::vector<char>> blobs(3);
    tmac_ggml_tensor w[3];
    for (int m = 0; m < 3; ++m) {
        blobs[m] = slurp(d + "/blob_" + names[m] + ".bin");
        w[m] = tmac_ggml_tensor{{cols[m], rows[m], 1, 1}, blobs[m].data(), nullptr};
        if (!ggml_tmac_hip_can_mul_mat(&w[m], bits)) { fprintf(stderr, "no kcfg entry for %s\n", names[m]); return 4; }
        CK(ggml_tmac_hip_upload(&w[m], bits));
    }
    void* x = dev(slurp(d + "/x.bin"));
    float* h = (float*)dev(slurp(d + "/h.bin"));
    float* g = (float*)dev(slurp(d + "/g.bin"));
    float* t = (float*)dzero(sizeof(float) * (size_t)N * H);
    void *gu[2] = {dzero(2 * (size_t)N * F), dzero(2 * (size_t)N * F)}, *dn = dzero(sizeof(float) * (size_t)N * H);
    const tmac_ggml_tensor *wgu[2] = {&w[0], &w[1]}, *wd[1] = {&w[2]};
    CK(ggml_tmac_hip_mul_mat_dev_xf_rows(wgu, 2, x, 0, 1, nullptr, h, g, 1e-5f, t, gu, 0, N));                  // t = x + h; gate, up = W rmsnorm(t)
    CK(ggml_tmac_hip_mul_mat_dev_xf_rows(wd, 1, gu[0], 0, 2, gu[1], nullptr, nullptr, 0.f, nullptr, &dn, 1, N));   // down = W (silu(gate) * up), fp32
    CK(ggml_tmac_hip_synchronize());
    // refusals reach the caller: an in-place residual stream, and a kind the glue does not know
    if (ggml_tmac_hip_mul_mat_dev_xf_rows(wgu, 2, x, 0, 1, nullptr, h, g, 1e-5f, h, gu, 0, N) == 0) { fprintf(stderr, "in-place residual accepted\n"); return 10; }
    if (ggml_tmac_hip_mul_mat_dev_xf_rows(wgu, 2, x, 0, 0, nullptr, nullptr, nullptr, 0.f, nullptr, gu, 0, N) == 0) { fprintf(stderr, "kind 0 accepted\n"); return 10; }
    CK(ggml_tmac_hip_synchronize());
    dump(d + "/out_t.bin", t, sizeof(float) * (size_t)N * H);
    dump(d + "/out_gate.bin", gu[0], 2 * (size_t)N * F);
    dump(d + "/out_up.bin", gu[1], 2 * (size_t)N * F);
    dump(d + "/out_down.bin", dn, sizeof(float) * (size_t)N * H);
    for (int m = 0; m < 3; ++m) ggml_tmac_hip_free(&w[m]);
    printf("RESULT ok\n");
    return 0;
}
