// fot_noise_emu.cpp -- csrc/fot_noise.hpp on the CPU: Philox4x32-10 on given counters and keys, and the noise tensor of
// fot_sgan_noise for given row tables.  Stand-alone (its own main), so that it can also be built with
// -fsanitize=address,undefined and run as it is.
//
//   fot_noise_emu philox <case.bin> <out.bin>
// case.bin: int32 n | uint32 [n][6] (c0 c1 c2 c3 k0 k1).  out.bin: uint32 [n][4].
//   fot_noise_emu noise <case.bin> <out.bin>
// case.bin: uint64 seed | int32 kind | int32 S | int32 rows | int32 noise_dim | int32 slot[rows] | int32 step[rows] |
// int32 index[rows].  out.bin: 32-bit words [S][rows][noise_dim] (float32, or the raw uint32 words of kind 0).
//   fot_noise_emu values <case.bin> <out.bin>
// case.bin: int32 kind | int32 n | uint32 [n][4] blocks of words.  out.bin: 32-bit words [n][4], the blocks under `kind`.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../integrated_path_planning_amd/csrc/fot_noise.hpp"

namespace {
bool read_all(std::FILE *f, void *dst, size_t bytes) { return bytes == 0 || std::fread(dst, 1, bytes, f) == bytes; }

int write_words(const char *path, const std::vector<uint32_t> &out)
{
    std::FILE *o = std::fopen(path, "wb");
    if (!o) { std::perror(path); return 2; }
    if (!out.empty() && std::fwrite(out.data(), sizeof(uint32_t), out.size(), o) != out.size()) { std::perror("write"); return 2; }
    std::fclose(o);
    return 0;
}
}

int main(int argc, char **argv)
{
    if (argc != 4) { std::fprintf(stderr, "usage: %s philox|noise|values case.bin out.bin\n", argv[0]); return 2; }
    std::FILE *in = std::fopen(argv[2], "rb");
    if (!in) { std::perror(argv[2]); return 2; }
    std::vector<uint32_t> out;
    if (std::strcmp(argv[1], "philox") == 0) {
        int32_t n = 0;
        if (!read_all(in, &n, sizeof n) || n < 0) { std::fprintf(stderr, "bad header\n"); return 2; }
        std::vector<uint32_t> c((size_t)n * 6);
        if (!read_all(in, c.data(), sizeof(uint32_t) * c.size())) { std::fprintf(stderr, "truncated\n"); return 2; }
        out.resize((size_t)n * 4);
        for (int i = 0; i < n; ++i) {
            const uint32_t *q = c.data() + 6 * (size_t)i;
            const fot::NoiseBlock b = fot::philox4x32_10(q[0], q[1], q[2], q[3], q[4], q[5]);
            for (int j = 0; j < 4; ++j) out[4 * (size_t)i + j] = b.w[j];
        }
    } else if (std::strcmp(argv[1], "noise") == 0) {
        uint64_t seed = 0;
        int32_t hdr[4] = { 0, 0, 0, 0 };
        if (!read_all(in, &seed, sizeof seed) || !read_all(in, hdr, sizeof hdr)) { std::fprintf(stderr, "bad header\n"); return 2; }
        const int kind = hdr[0], S = hdr[1], rows = hdr[2], nd = hdr[3];
        if (kind < 0 || kind >= fot::NOISE_KINDS || S < 0 || rows < 0 || nd < 0) { std::fprintf(stderr, "bad shape\n"); return 2; }
        std::vector<int32_t> slot((size_t)rows), step((size_t)rows), idx((size_t)rows);
        if (!read_all(in, slot.data(), 4 * slot.size()) || !read_all(in, step.data(), 4 * step.size()) ||
            !read_all(in, idx.data(), 4 * idx.size())) { std::fprintf(stderr, "truncated tables\n"); return 2; }
        out.resize((size_t)S * rows * nd);
        for (int s = 0; s < S; ++s)
            for (int r = 0; r < rows; ++r)
                for (int b = 0; 4 * b < nd; ++b) {
                    uint32_t v[4];
                    fot::noise_values(fot::noise_block(seed, slot[(size_t)r], step[(size_t)r], idx[(size_t)r], s, b), kind, v);
                    for (int j = 0; j < 4 && 4 * b + j < nd; ++j) out[((size_t)s * rows + r) * nd + 4 * b + j] = v[j];
                }
    } else if (std::strcmp(argv[1], "values") == 0) {
        int32_t hdr[2] = { 0, 0 };
        if (!read_all(in, hdr, sizeof hdr) || hdr[0] < 0 || hdr[0] >= fot::NOISE_KINDS || hdr[1] < 0) { std::fprintf(stderr, "bad header\n"); return 2; }
        std::vector<uint32_t> w((size_t)hdr[1] * 4);
        if (!read_all(in, w.data(), sizeof(uint32_t) * w.size())) { std::fprintf(stderr, "truncated\n"); return 2; }
        out.resize(w.size());
        for (int i = 0; i < hdr[1]; ++i) {
            fot::NoiseBlock b;
            for (int j = 0; j < 4; ++j) b.w[j] = w[4 * (size_t)i + j];
            fot::noise_values(b, hdr[0], out.data() + 4 * (size_t)i);
        }
    } else {
        std::fprintf(stderr, "unknown mode %s\n", argv[1]);
        return 2;
    }
    std::fclose(in);
    return write_words(argv[3], out);
}
