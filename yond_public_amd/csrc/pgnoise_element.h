// The value yond_pg_noise_f32 stores for one element (include/yond_hip.h I2), shared by pgnoise.hip, which stores it, and noisehist.hip,
// which bins its residual without storing it: one definition, so the two agree bit for bit.
#pragma once
#include "common.h"
#include "pgnoise_sampler.h"

__device__ __forceinline__ float pg_element(const YondPGItem& it, uint64_t index, float x, int clip) {
    if (!(fabsf(x) <= 3.402823466e38f)) return __builtin_nanf("");        // NaN, +-inf
    const float e = it.exposure, beta1 = it.beta1;
    const float xp = fmaxf(x, 0.0f);
    const bool shot = beta1 > 0.0f;
    float lam = shot ? xp * e / beta1 : 0.0f;
    const bool huge = !(lam <= 3.402823466e38f);                            // x e / beta1 overflowed: the count is not representable,
    if (huge) lam = 0.0f;                                                   // its relative noise is nil
    const PGDraw d = pg_draw(it.key, it.slot, index, lam);
    const float signal = (shot && !huge) ? (d.k * beta1) / e : xp;
    float y = signal + fminf(x, 0.0f) + it.sigma_n * d.z / e;
    y = fminf(fmaxf(y, -3.402823466e38f), 3.402823466e38f);                // a finite x never gives an infinity
    if (clip) y = fminf(fmaxf(y, 0.0f), 1.0f);
    return y;
}
