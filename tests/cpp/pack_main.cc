// pack_main.cc — packs one matrix on the host through tmac_amd/csrc/tmac_pack.h, the index and nibble arithmetic the pack kernels
// (tmac_pack.hip) share: every (weight row, plane, table) goes through the same functions a GPU thread calls.  Plain g++, no HIP.
//   pack_main gptq  Mw K bits bm kfactor gs zero_point gptq_v2 scales_f16 out_f16 qweight.bin scales.bin qzeros.bin A.bin S.bin
//   pack_main codes Mw K bits bm kfactor gs zero_point 0       scales_f16 out_f16 codes.bin   scales.bin zeros.bin  A.bin S.bin
// Inputs in the layouts of include/tmac_hip.h ("device-side packing"); outputs the two halves of the reference blob.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
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
    if (argc != 17) { fprintf(stderr, "usage: see the head of pack_main.cc\n"); return 2; }
    const bool gptq = std::string(argv[1]) == "gptq";
    const int Mw = atoi(argv[2]), K = atoi(argv[3]), bits = atoi(argv[4]), bm = atoi(argv[5]), kf = atoi(argv[6]), gs = atoi(argv[7]);
    const int zp = atoi(argv[8]), v2 = atoi(argv[9]), sf16 = atoi(argv[10]), of16 = atoi(argv[11]);
    const int T = K / 4, SG = K / gs, M = Mw * bits;
    const std::vector<uint8_t> wsrc = slurp(argv[12]);
    Floats sc{slurp(argv[13]), sf16 != 0};
    const std::vector<uint8_t> zsrc = zp ? slurp(argv[14]) : std::vector<uint8_t>();
    need(sc.raw, (size_t)Mw * SG * (sf16 ? 2 : 4), "scales");

    std::vector<uint8_t> A((size_t)M * T / 2, 0);
    auto put = [&](int o, int p, int t, uint32_t nib) {
        const int r = pk::mrow(o, p, bits);
        A[pk::blob_byte(r, t, bm, kf, T)] |= (uint8_t)(nib << (pk::blob_high(r, bm) ? 4 : 0));
    };
    if (gptq) {
        const int per = 32 / bits, tables = 8 / bits;
        need(wsrc, (size_t)(K / per) * Mw * 4, "qweight");
        for (int kp = 0; kp < K / per; ++kp)
            for (int m = 0; m < Mw; ++m) {
                uint32_t word;
                memcpy(&word, wsrc.data() + 4 * ((size_t)kp * Mw + m), 4);
                for (int p = 0; p < bits; ++p) {
                    const uint32_t v = pk::gptq_plane(word, p, bits);
                    for (int i = 0; i < tables; ++i) put(m, p, kp * tables + i, (v >> (4 * i)) & 15u);
                }
            }
    } else {
        need(wsrc, (size_t)Mw * K, "codes");
        for (int o = 0; o < Mw; ++o)
            for (int t = 0; t < T; ++t) {
                uint32_t four;
                memcpy(&four, wsrc.data() + (size_t)o * K + 4 * t, 4);
                for (int p = 0; p < bits; ++p) put(o, p, t, pk::codes_nibble(four, p));
            }
    }

    Floats S{std::vector<uint8_t>((size_t)Mw * SG * (zp ? 2 : 1) * (of16 ? 2 : 4), 0), of16 != 0};
    if (zp) need(zsrc, gptq ? (size_t)SG * (M / 32) * 4 : (size_t)Mw * SG * (sf16 ? 2 : 4), gptq ? "qzeros" : "zeros");
    Floats zr{gptq ? std::vector<uint8_t>() : zsrc, sf16 != 0};
    for (int sg = 0; sg < SG; ++sg)
        for (int o = 0; o < Mw; ++o) {
            const float s = sc.get(gptq ? (size_t)sg * Mw + o : (size_t)o * SG + sg);
            S.set(pk::scale_index(o, sg, 0, bm, bits, SG, zp), s);
            if (!zp) continue;
            float z;
            if (gptq) {
                uint32_t word;
                memcpy(&word, zsrc.data() + 4 * ((size_t)sg * (M / 32) + (size_t)o * bits / 32), 4);
                z = pk::gptq_zero_multiplier(pk::gptq_field(word, o % (32 / bits), bits), v2 ? 0 : 1, bits) * s;
                if (sf16) z = pk::round_to_f16(z);      // one rounding, to the scales' dtype
            } else {
                z = zr.get((size_t)o * SG + sg);
            }
            S.set(pk::scale_index(o, sg, 1, bm, bits, SG, zp), z);
        }
    dump(argv[15], A.data(), A.size());
    dump(argv[16], S.raw.data(), S.raw.size());
    return 0;
}
