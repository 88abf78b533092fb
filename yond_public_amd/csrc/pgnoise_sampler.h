// The per-element sampler of pgnoise.hip: one Poisson count and one standard normal from Philox4x32-10, as a function of
// (key, slot, element index, lambda) and of nothing else.  Plain C++ too (philox.h): tests/pgnoise_host_sampler.cpp runs it on the CPU (tests/test_pgnoise_host.py).
//
// Counter (c0, c1, c2, c3) = (index low, index high, draw number, PG_TAG).  Draw 0 gives the Box-Muller pair (words 0, 1: z for the read
// noise, zn for the normal regime) and the first Poisson attempt (words 2, 3); draw j >= 1 gives attempts 2j - 1 and 2j.
//
// Regimes by lambda (PG_SWITCH_*; yond_public_amd/pgnoise.py SWITCH_LAMBDAS repeats them):
//   lambda <  10            inversion: sequential search of the CDF with one 24-bit uniform, float32.  At most PG_INV_MAX steps; the
//                           search also stops where a term falls below 2^-26 past the mode (nothing a 24-bit uniform can resolve).
//   10 <= lambda <= 2^23    PTRS (W. Hoermann, "The transformed rejection method for generating Poisson random variables", Insurance:
//                           Mathematics and Economics 12, 1993).  The acceptance test needs log f(k) = -lambda + k log lambda - log k!,
//                           whose terms reach 1e8 and cancel to O(10): it is evaluated as a Stirling difference instead, with
//                           d = k - lambda, x = d / lambda:
//                               log f(k) = -d^2 / lambda + k (x - log1p(x)) - log(2 pi k) / 2 - (1/(12k) - 1/(360k^3) + 1/(1260k^5))
//                           where x - log1p(x) = s x - 2 s^3 (1/3 + s^2/5 + ...), s = x / (2 + x), for |x| <= 0.3: no term is larger
//                           than the result, float32 holds it to ~1e-6 absolute.  k < 10 uses a table of log k!.
//                           At most PG_MAX_ATTEMPTS attempts (each accepts with probability > 0.85), then the normal regime.
//   lambda >  2^23          counts no longer fit float32 exactly: max(0, rint(lambda + sqrt(lambda) zn)).
// Every loop has a fixed trip bound; a non-finite or non-positive lambda never enters one.
#pragma once
#include "philox.h"

#define PG_TAG 0x50474e31u                 /* "PGN1": keeps these streams apart from img2raw's (counter word 3 = 0 there) */
#define PG_SWITCH_PTRS 10.0f
#define PG_SWITCH_NORMAL 8388608.0f        /* 2^23 */
#define PG_INV_MAX 64
#define PG_MAX_ATTEMPTS 64

// x - log1p(x) for x > -1
YOND_RNG_FN float pg_x_minus_log1p(float x) {
    if (fabsf(x) > 0.3f) return x - log1pf(x);
    const float s = x / (2.0f + x), t = s * s;
    float p = 1.0f / 15.0f;
    p = p * t + 1.0f / 13.0f;
    p = p * t + 1.0f / 11.0f;
    p = p * t + 1.0f / 9.0f;
    p = p * t + 1.0f / 7.0f;
    p = p * t + 1.0f / 5.0f;
    p = p * t + 1.0f / 3.0f;
    return s * x - 2.0f * (s * t) * p;
}

// log of the Poisson probability of k (an integer >= 0 held as float) at lam >= PG_SWITCH_PTRS
YOND_RNG_FN float pg_log_pmf(float k, float lam, float loglam) {
    if (k < 10.0f) {
        const float lf[10] = {0.0f, 0.0f, 0.69314718f, 1.79175947f, 3.17805383f, 4.78749174f, 6.57925121f, 8.52516136f, 10.60460290f,
                              12.80182748f};
        float l = 0.0f;
#pragma unroll
        for (int j = 0; j < 10; ++j) l = (k == (float)j) ? lf[j] : l;      // selects, not an indexed array: no scratch
        return k * loglam - lam - l;
    }
    const float d = k - lam, x = d / lam, rk = 1.0f / k, rk2 = rk * rk;
    const float stirling = rk * (1.0f / 12.0f - rk2 * (1.0f / 360.0f - rk2 * (1.0f / 1260.0f)));
    return k * pg_x_minus_log1p(x) - d * x - 0.5f * logf(6.283185307179586f * k) - stirling;
}

struct PGDraw { float k, z; };

// the normal regime's count: formed in float64, a float32 sum above 2^23 would round before rint
YOND_RNG_FN float pg_normal_count(float lam, float slam, float zn) {
    return (float)fmax(0.0, rint((double)lam + (double)slam * (double)zn));
}

// k ~ Poisson(lam) for finite lam >= 0 (as float: integers beyond 2^24 are the nearest float), z ~ N(0, 1) independent of k
YOND_RNG_FN PGDraw pg_draw(uint32_t key, uint32_t slot, uint64_t index, float lam) {
    const uint32_t c0 = (uint32_t)index, c1 = (uint32_t)(index >> 32);
    Philox4 r = philox4x32_10(c0, c1, 0u, PG_TAG, key, slot);
    PGDraw out;
    float zn;
    box_muller(r.v[0], r.v[1], out.z, zn);
    out.k = 0.0f;
    if (!(lam > 0.0f)) return out;
    if (lam < PG_SWITCH_PTRS) {
        const float u = (float)(r.v[2] >> 8) * 5.9604644775390625e-8f;       // [0, 1)
        float p = expf(-lam), cdf = p, k = 0.0f;
        for (int it = 0; it < PG_INV_MAX; ++it) {
            if (u < cdf || (k > lam && p < 1.4901161e-8f)) break;
            k += 1.0f;
            p = p * lam / k;
            cdf += p;
        }
        out.k = k;
        return out;
    }
    const float slam = sqrtf(lam);
    if (lam > PG_SWITCH_NORMAL) {
        out.k = pg_normal_count(lam, slam, zn);
        return out;
    }
    const float loglam = logf(lam);
    const float b = 0.931f + 2.53f * slam;
    const float a = -0.059f + 0.02483f * b;
    const float inv_alpha = 1.1239f + 1.1328f / (b - 3.4f);
    const float vr = 0.9277f - 3.6224f / (b - 2.0f);
    for (int att = 0; att < PG_MAX_ATTEMPTS; ++att) {
        if (att & 1) r = philox4x32_10(c0, c1, (uint32_t)((att + 1) >> 1), PG_TAG, key, slot);
        const uint32_t wu = (att & 1) ? r.v[0] : r.v[2], wv = (att & 1) ? r.v[1] : r.v[3];
        const float U = ((float)(int32_t)((wu >> 8) - 8388608u) + 0.5f) * 5.9604644775390625e-8f;     // (-0.5, 0.5), never 0
        const float V = (float)((wv >> 8) + 1u) * 5.9604644775390625e-8f;                             // (0, 1]
        const float us = 0.5f - fabsf(U);
        const double kd = floor((double)((2.0f * a / us + b) * U) + (double)lam + 0.43);
        const float k = (float)kd;
        if (us >= 0.07f && V <= vr) {
            out.k = k;
            return out;
        }
        if (kd < 0.0 || (us < 0.013f && V > us)) continue;
        if (logf(V * inv_alpha / (a / (us * us) + b)) <= pg_log_pmf(k, lam, loglam)) {
            out.k = k;
            return out;
        }
    }
    out.k = pg_normal_count(lam, slam, zn);    // every attempt refused (probability < 0.15^64): the normal regime's value
    return out;
}
