// Philox4x32-10 (Salmon et al., "Parallel Random Numbers: As Easy as 1, 2, 3", SC 2011) and Box-Muller on its words: the counter-based
// noise source of img2raw.hip and pgnoise.hip.  The file also compiles as plain C++ (no HIP): tests/pgnoise_host_sampler.cpp runs the
// Poisson sampler of pgnoise_sampler.h on the CPU (tests/test_pgnoise_host.py).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define YOND_RNG_FN __host__ __device__ __forceinline__
#else
#define YOND_RNG_FN static inline
#endif

struct Philox4 { uint32_t v[4]; };

YOND_RNG_FN uint32_t yond_mulhi32(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umulhi(a, b);
#else
    return (uint32_t)(((uint64_t)a * b) >> 32);
#endif
}

YOND_RNG_FN Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t lo0 = 0xD2511F53u * c0, hi0 = yond_mulhi32(0xD2511F53u, c0);
        const uint32_t lo1 = 0xCD9E8D57u * c2, hi1 = yond_mulhi32(0xCD9E8D57u, c2);
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return Philox4{{c0, c1, c2, c3}};
}

// Box-Muller on two 32-bit words: u1 in (0, 1] (24 bits), u2 in [0, 1)
YOND_RNG_FN void box_muller(uint32_t a, uint32_t b, float& z0, float& z1) {
    const float u1 = (float)((a >> 8) + 1u) * 5.9604644775390625e-8f;
    const float u2 = (float)(b >> 8) * 5.9604644775390625e-8f;
    const float r = sqrtf(-2.0f * logf(u1));
    float s, c;
#if defined(__HIP_DEVICE_COMPILE__)
    sincospif(2.0f * u2, &s, &c);
#else
    s = sinf(6.283185307179586f * u2);       // the host C library has no sincospif: same law, other last bits
    c = cosf(6.283185307179586f * u2);
#endif
    z0 = r * c;
    z1 = r * s;
}
