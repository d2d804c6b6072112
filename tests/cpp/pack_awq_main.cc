// pack_awq_main.cc — packs one AutoAWQ GEMM matrix on the host through tmac_amd/csrc/tmac_pack.h, the index and nibble arithmetic the
// pack kernels (tmac_pack.hip) share: the AWQ field rule (awq_field_of_row, awq_row_of_field, awq_code) and the plane extraction of
// k_pack_awq_weights' stage 1 (awq_plane_byte), then the blob addresses every packer uses.  Plain g++, no HIP.
//   pack_awq_main Mw K bm kfactor gs zero_point scales_f16 out_f16 qweight.bin scales.bin qzeros.bin A.bin S.bin
// Inputs in the layouts of include/tmac_hip.h ("AutoAWQ checkpoints"); outputs the two halves of the reference blob.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../tmac_amd/csrc/tmac_pack.h"

namespace pk = tmac_pack;

static std::vector<uint8_t> slurp(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    std::vector<uint8_t> v;
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return v;
}
static void dump(const char* path, const void* p, size_t n) {
    FILE* f = fopen(path, "wb");
    if (!f || fwrite(p, 1, n, f) != n) { fprintf(stderr, "cannot write %s\n", path); exit(2); }
    fclose(f);
}
static void need(const std::vector<uint8_t>& v, size_t bytes, const char* what) {
    if (v.size() != bytes) { fprintf(stderr, "%s: %zu bytes, %zu expected\n", what, v.size(), bytes); exit(2); }
}

struct Floats {     // an fp16 or fp32 array behind one interface
    std::vector<uint8_t> raw;
    bool f16;
    float get(size_t i) const {
        if (f16) { uint16_t h; memcpy(&h, raw.data() + 2 * i, 2); return pk::f16_bits_to_f32(h); }
        float v; memcpy(&v, raw.data() + 4 * i, 4); return v;
    }
    void set(size_t i, float v) {
        if (f16) { const uint16_t h = pk::f32_to_f16_bits(v); memcpy(raw.data() + 2 * i, &h, 2); }
        else memcpy(raw.data() + 4 * i, &v, 4);
    }
};

int main(int argc, char** argv) {
    if (argc != 14) { fprintf(stderr, "usage: see the head of pack_awq_main.cc\n"); return 2; }
    const int Mw = atoi(argv[1]), K = atoi(argv[2]), bm = atoi(argv[3]), kf = atoi(argv[4]), gs = atoi(argv[5]);
    const int zp = atoi(argv[6]), sf16 = atoi(argv[7]), of16 = atoi(argv[8]);
    const int bits = 4, T = K / 4, SG = K / gs, M = Mw * bits, MO = Mw / 8;
    const std::vector<uint8_t> wsrc = slurp(argv[9]);
    Floats sc{slurp(argv[10]), sf16 != 0};
    const std::vector<uint8_t> zsrc = zp ? slurp(argv[11]) : std::vector<uint8_t>();
    need(wsrc, (size_t)K * MO * 4, "qweight");
    need(sc.raw, (size_t)Mw * SG * (sf16 ? 2 : 4), "scales");
    if (zp) need(zsrc, (size_t)SG * MO * 4, "qzeros");
    for (int i = 0; i < 8; ++i)
        if (pk::awq_field_of_row(pk::awq_row_of_field(i)) != i) { fprintf(stderr, "the field rule is no permutation\n"); return 3; }
    auto word = [&](const std::vector<uint8_t>& src, size_t i) { uint32_t w; memcpy(&w, src.data() + 4 * i, 4); return w; };

    std::vector<uint8_t> A((size_t)M * T / 2, 0);
    auto put = [&](int o, int p, int t, uint32_t nib) {
        const int r = pk::mrow(o, p, bits);
        A[pk::blob_byte(r, t, bm, kf, T)] |= (uint8_t)(nib << (pk::blob_high(r, bm) ? 4 : 0));
    };
    // as stage 1 of the kernel: (octet c, table pair tp) takes the eight words of columns 8 tp .. 8 tp + 7 (zeros past K) and makes the
    // byte of every (row of the octet, plane): the nibble of table 2 tp below the nibble of table 2 tp + 1
    for (int c = 0; c < MO; ++c)
        for (int tp = 0; tp < (T + 1) / 2; ++tp) {
            uint32_t w[8];
            for (int kk = 0; kk < 8; ++kk) w[kk] = 8 * tp + kk < K ? word(wsrc, (size_t)(8 * tp + kk) * MO + c) : 0u;
            uint32_t lo[4], hi[4];
            for (int p = 0; p < bits; ++p) {
                lo[p] = pk::awq_plane_nibbles(w[0], w[1], w[2], w[3], p);
                hi[p] = pk::awq_plane_nibbles(w[4], w[5], w[6], w[7], p);
            }
            for (int j = 0; j < 8; ++j) {
                for (int p = 0; p < bits; ++p) {
                    const uint32_t b = pk::awq_plane_byte(lo[p], hi[p], j);
                    put(8 * c + j, p, 2 * tp, b & 15u);
                    if (2 * tp + 1 < T) put(8 * c + j, p, 2 * tp + 1, b >> 4);
                }
                // the same codes through the one-code accessor
                for (int kk = 0; kk < 8; ++kk) {
                    uint32_t code = 0;
                    for (int p = 0; p < bits; ++p) code |= ((pk::awq_plane_byte(lo[p], hi[p], j) >> kk) & 1u) << p;
                    if (code != pk::awq_code(w[kk], j)) { fprintf(stderr, "awq_plane_byte and awq_code disagree\n"); return 3; }
                }
            }
        }

    Floats S{std::vector<uint8_t>((size_t)Mw * SG * (zp ? 2 : 1) * (of16 ? 2 : 4), 0), of16 != 0};
    for (int sg = 0; sg < SG; ++sg)
        for (int o = 0; o < Mw; ++o) {
            const float s = sc.get((size_t)sg * Mw + o);
            S.set(pk::scale_index(o, sg, 0, bm, bits, SG, zp), s);
            if (!zp) continue;
            float z = pk::gptq_zero_multiplier(pk::awq_code(word(zsrc, (size_t)sg * MO + o / 8), o % 8), 0, bits) * s;
            if (sf16) z = pk::round_to_f16(z);      // one rounding, to the scales' dtype
            S.set(pk::scale_index(o, sg, 1, bm, bits, SG, zp), z);
        }
    dump(argv[12], A.data(), A.size());
    dump(argv[13], S.raw.data(), S.raw.size());
    return 0;
}
