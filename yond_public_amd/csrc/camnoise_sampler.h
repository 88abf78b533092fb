// The per-element sampler of camnoise.hip: the draws of the camera noise model (data_process/process.py:631-671) that the Poisson-Gaussian
// sampler does not already make.  Plain C++ too (philox.h): tests/camnoise_host_sampler.cpp runs it on the CPU (tests/test_camnoise_host.py).
//
// Shot count and Gaussian read normal: pg_draw of pgnoise_sampler.h, unchanged -- counter (index low, index high, draw, PG_TAG).  With every
// other term off an element is therefore the Poisson-Gaussian kernel's, bit for bit.
// Element draw, counter (index low, index high, 0, CAM_TAG), one Philox4x32-10 call:
//   word 0          the Tukey-lambda uniform u = (w + 1) 2^-33 in [2^-33, 1/2] (32 bits; float32 keeps 24 of them RELATIVE to u, so the
//                   tail is resolved as finely as the centre)
//   word 1 bit 0    its sign: the law is symmetric, the variate is -+ Q_lam(u)
//   word 2          the quantisation uniform, ((w >> 9) + 0.5) 2^-23 - 0.5: 2^23 levels in (-0.5, 0.5), symmetric, never +-0.5
//   words 3, 1      Box-Muller (bits 8.. of each): the normal of the Gaussian shot approximation
// Row draw, counter (row low, row high, 0, CAM_ROW_TAG): Box-Muller on words 0, 1.  A function of (key, slot, row) alone: every element
// of a row computes the same float.
//
// Tukey-lambda quantile Q_lam(u) = (u^lam - (1 - u)^lam) / lam (scipy.stats.tukeylambda.ppf), evaluated as
//     (expm1(lam log u) - expm1(lam log1p(-u))) / lam
// so that a small |lam| does not cancel (the two powers are 1 + O(lam)); lam == 0 exactly is the logistic log u - log1p(-u).
// Tail truncation: u >= 2^-33, so |Q| <= |Q_lam(2^-33)|: 1468 at lam = -0.26, 22.9 at lam = 0, 8.85 at lam = 0.102.  The mass beyond is
// 2^-32 in all; for lam > 0 the law is bounded by 1 / lam anyway.  The result is clamped to the finite floats: a lam no caller should
// pass (below -3.8 the power overflows) gives +-FLT_MAX, never an infinity or a NaN.
// No loop at all in this file; pg_draw's have fixed bounds.
#pragma once
#include "pgnoise_sampler.h"

#define CAM_TAG 0x43414d31u                /* "CAM1" */
#define CAM_ROW_TAG 0x43524f57u            /* "CROW" */

// Q_lam(u) for u in (0, 1/2]: <= 0
YOND_RNG_FN float cam_tl_quantile(float lam, float u) {
    const float lu = logf(u), l1u = log1pf(-u);
    float q;
    if (lam == 0.0f) q = lu - l1u;
    else q = (expm1f(lam * lu) - expm1f(lam * l1u)) / lam;
    return fminf(fmaxf(q, -3.402823466e38f), 3.402823466e38f);
}

struct CamDraw {
    float tl;      // Tukey-lambda(lam) variate, scale 1
    float uq;      // uniform on (-0.5, 0.5)
    float zs;      // N(0, 1)
};

YOND_RNG_FN CamDraw cam_draw(uint32_t key, uint32_t slot, uint64_t index, float lam) {
    const Philox4 r = philox4x32_10((uint32_t)index, (uint32_t)(index >> 32), 0u, CAM_TAG, key, slot);
    CamDraw d;
    const float u = ((float)r.v[0] + 1.0f) * 1.16415321826934814453125e-10f;       // 2^-33: [2^-33, 1/2]
    const float q = cam_tl_quantile(lam, u);
    d.tl = (r.v[1] & 1u) ? -q : q;
    d.uq = ((float)(r.v[2] >> 9) + 0.5f) * 1.1920928955078125e-7f - 0.5f;        // 23 bits: k + 0.5 is exact
    float unused;
    box_muller(r.v[3], r.v[1], d.zs, unused);
    return d;
}

YOND_RNG_FN float cam_row_normal(uint32_t key, uint32_t slot, uint64_t row) {
    const Philox4 r = philox4x32_10((uint32_t)row, (uint32_t)(row >> 32), 0u, CAM_ROW_TAG, key, slot);
    float z, unused;
    box_muller(r.v[0], r.v[1], z, unused);
    return z;
}
