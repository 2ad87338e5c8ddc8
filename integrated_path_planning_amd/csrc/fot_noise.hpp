// fot_noise.hpp -- the counter-based noise of the Social-GAN sampler (fot_sgan_noise, fot_loop_set_sampler): Philox4x32-10
// and the maps from its words to uniform and Gaussian numbers.  Plain C++, no HIP: the kernel (fot_sgan.hip) and the CPU
// emulation (tests/emu/fot_noise_emu.cpp) compile the same arithmetic; tests/noise_common.py restates it in NumPy.
//
// A number is a function of (seed, slot, step, p, s, d) alone: key = the 64-bit seed (low word first), counter =
// { d / 4, p | (s << 16), step, slot }; one block yields the numbers of dimensions 4 (d / 4) .. 4 (d / 4) + 3.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FOT_NOISE_HD __host__ __device__
#else
#define FOT_NOISE_HD
#endif

namespace fot {

struct NoiseBlock {
    uint32_t w[4];
};

FOT_NOISE_HD inline void philox_mulhilo(uint32_t a, uint32_t b, uint32_t &hi, uint32_t &lo)
{
    const uint64_t p = (uint64_t)a * (uint64_t)b;
    hi = (uint32_t)(p >> 32); lo = (uint32_t)p;
}

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; Random123's philox4x32_R(10, ...))
FOT_NOISE_HD inline NoiseBlock philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
    for (int r = 0; r < 10; ++r) {
        uint32_t hi0, lo0, hi1, lo1;
        philox_mulhilo(0xD2511F53u, c0, hi0, lo0);
        philox_mulhilo(0xCD9E8D57u, c2, hi1, lo1);
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    NoiseBlock b;
    b.w[0] = c0; b.w[1] = c1; b.w[2] = c2; b.w[3] = c3;
    return b;
}

// the block of (seed, slot, step, p, s, b = d / 4)
FOT_NOISE_HD inline NoiseBlock noise_block(uint64_t seed, int32_t slot, int32_t step, int32_t p, int32_t s, int32_t b)
{
    return philox4x32_10((uint32_t)b, (uint32_t)p | ((uint32_t)s << 16), (uint32_t)step, (uint32_t)slot, (uint32_t)seed,
                         (uint32_t)(seed >> 32));
}

// [0, 1): the word's upper 24 bits (torch's rand for float32)
FOT_NOISE_HD inline float noise_uniform(uint32_t x) { return (float)(x >> 8) * 0x1p-24f; }

// [-1, 1): what the reference makes of a uniform draw (sgan_vendor/models.py get_noise: (rand - 0.5) * 2); both steps exact
FOT_NOISE_HD inline float noise_uniform_sym(uint32_t x) { return (noise_uniform(x) - 0.5f) * 2.0f; }

// Box-Muller on a pair of words, in float64, rounded once: u1 in (0, 1] (no logarithm of 0), u2 in [0, 1)
FOT_NOISE_HD inline void noise_gauss_pair(uint32_t xa, uint32_t xb, float &g0, float &g1)
{
    const double u1 = (double)((xa >> 8) + 1u) * 0x1p-24, u2 = (double)(xb >> 8) * 0x1p-24;
    const double l = log(u1);
    const double r = sqrt(-2.0 * l);
    const double a = 6.283185307179586 * u2;
    const double c = r * cos(a), s = r * sin(a);
    g0 = (float)c; g1 = (float)s;
}

// kinds of fot_sgan_noise (include/fot.h FOT_NOISE_*)
constexpr int NOISE_RAW = 0, NOISE_UNIFORM = 1, NOISE_GAUSSIAN = 2, NOISE_UNIFORM_SYM = 3, NOISE_KINDS = 4;

// the four 32-bit results of one block under `kind` (NOISE_RAW: the words themselves)
FOT_NOISE_HD inline void noise_values(const NoiseBlock &b, int kind, uint32_t out[4])
{
    float f[4];
    if (kind == NOISE_GAUSSIAN) {
        noise_gauss_pair(b.w[0], b.w[1], f[0], f[1]);
        noise_gauss_pair(b.w[2], b.w[3], f[2], f[3]);
    } else if (kind == NOISE_UNIFORM) {
        for (int j = 0; j < 4; ++j) f[j] = noise_uniform(b.w[j]);
    } else if (kind == NOISE_UNIFORM_SYM) {
        for (int j = 0; j < 4; ++j) f[j] = noise_uniform_sym(b.w[j]);
    } else {
        for (int j = 0; j < 4; ++j) out[j] = b.w[j];
        return;
    }
    for (int j = 0; j < 4; ++j) {
        union { float f; uint32_t u; } v;
        v.f = f[j];
        out[j] = v.u;
    }
}

}  // namespace fot
