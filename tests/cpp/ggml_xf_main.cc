// One llama-shaped layer, call by call, through the ggml glue's device-resident mat-muls (include/ggml-tmac-hip.h): q/k/v behind an
// RMSNorm, o, gate/up behind [+ residual, RMSNorm], down behind [silu(gate) * up], the next q/k/v behind [+ residual, RMSNorm] -- the
// element-wise operators inside the kernels (ggml_tmac_hip_mul_mat_dev_xf), the residual stream alternating between two buffers, an
// operator outside the hook between q/k/v and o (a device copy on the glue's stream: the stand-in for attention).  Every tensor is
// dumped; tests/test_gpu_ggml_xf.py recomputes each stage with the oracle.
// usage: ggml_xf_main <dir> H F bits      (dir: kcfg.ini, blob_<name>.bin, h0.bin (fp32 [H]), g1.bin, g2.bin, g3.bin (fp32 [H]))
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "ggml-tmac-hip.h"

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
    float* hbuf[2] = {(float*)dev(slurp(d + "/h0.bin")), (float*)dzero(sizeof(float) * H)};      // the residual stream: two alternating buffers
    float* g[3];
    for (int k = 0; k < 3; ++k) g[k] = (float*)dev(slurp(d + "/g" + std::to_string(k + 1) + ".bin"));
    void* attn = dzero(2 * (size_t)H);
    void *qkv[3], *qkv2[3], *o = dzero(2 * (size_t)H), *gu[2] = {dzero(2 * (size_t)F), dzero(2 * (size_t)F)}, *dn = dzero(2 * (size_t)H);
    for (int k = 0; k < 3; ++k) { qkv[k] = dzero(2 * (size_t)H); qkv2[k] = dzero(sizeof(float) * H); }
    const tmac_ggml_tensor *wqkv[3] = {&w[0], &w[1], &w[2]}, *wo[1] = {&w[3]}, *wgu[2] = {&w[4], &w[5]}, *wd[1] = {&w[6]};
    // q/k/v from the fp32 embedding: RMSNorm only
    CK(ggml_tmac_hip_mul_mat_dev_xf(wqkv, 3, hbuf[0], 1, 1, nullptr, nullptr, g[0], 1e-5f, nullptr, qkv, 0));
    // the operator outside the hook, on the glue's stream: attn = q
    if (hipMemcpyAsync(attn, qkv[0], 2 * (size_t)H, 3, ggml_tmac_hip_stream())) return 9;
    CK(ggml_tmac_hip_mul_mat_dev(wo, 1, attn, 0, &o, 0));
    CK(ggml_tmac_hip_mul_mat_dev_xf(wgu, 2, o, 0, 1, nullptr, hbuf[0], g[1], 1e-5f, hbuf[1], gu, 0));           // t2 = o + h0 -> hbuf[1]
    CK(ggml_tmac_hip_mul_mat_dev_xf(wd, 1, gu[0], 0, 2, gu[1], nullptr, nullptr, 0.f, nullptr, &dn, 0));        // silu(gate) * up
    CK(ggml_tmac_hip_mul_mat_dev_xf(wqkv, 3, dn, 0, 1, nullptr, hbuf[1], g[2], 1e-5f, hbuf[0], qkv2, 1));       // t3 = down + t2 -> hbuf[0]; fp32 outputs
    CK(ggml_tmac_hip_synchronize());
    // refusals reach the caller: an in-place residual stream, and a kind the glue does not know
    if (ggml_tmac_hip_mul_mat_dev_xf(wgu, 2, o, 0, 1, nullptr, hbuf[1], g[1], 1e-5f, hbuf[1], gu, 0) == 0) { fprintf(stderr, "in-place residual accepted\n"); return 10; }
    if (ggml_tmac_hip_mul_mat_dev_xf(wgu, 2, o, 0, 0, nullptr, nullptr, nullptr, 0.f, nullptr, gu, 0) == 0) { fprintf(stderr, "kind 0 accepted\n"); return 10; }
    CK(ggml_tmac_hip_synchronize());
    dump(d + "/out_attn.bin", attn, 2 * (size_t)H);
    dump(d + "/out_t2.bin", hbuf[1], sizeof(float) * H);
    dump(d + "/out_t3.bin", hbuf[0], sizeof(float) * H);
    for (int k = 0; k < 3; ++k) {
        dump(d + "/out_" + names[k] + ".bin", qkv[k], 2 * (size_t)H);
        dump(d + "/out_next_" + names[k] + ".bin", qkv2[k], sizeof(float) * H);
    }
    dump(d + "/out_o.bin", o, 2 * (size_t)H);
    dump(d + "/out_gate.bin", gu[0], 2 * (size_t)F);
    dump(d + "/out_up.bin", gu[1], 2 * (size_t)F);
    dump(d + "/out_down.bin", dn, 2 * (size_t)H);
    for (int m = 0; m < 7; ++m) ggml_tmac_hip_free(&w[m]);
    printf("RESULT ok\n");
    return 0;
}
