// The sampler of csrc/pgnoise_sampler.h compiled for the CPU (tests/test_pgnoise_host.py test_sampler_on_the_cpu): the same source the kernel runs,
// with the host C library's logf / expf / sinf / cosf in place of the device's.
#include <stddef.h>

#include <math.h>
#include <stdint.h>
#include <string.h>

// -DYOND_NUDGE_ULPS=k (tests/noise_replay.py robust_mask): the four C-library functions whose last bits differ between the host and the
// device return their result moved k float32 ulps away from zero (k < 0: towards it).  A draw that survives k = +-4 does not hang on them.
#ifdef YOND_NUDGE_ULPS
static inline float yond_nudge(float x) {
    if (!(fabsf(x) <= 3.402823466e38f) || x == 0.0f) return x;
    uint32_t b;
    memcpy(&b, &x, 4);
    int64_t m = (int64_t)(b & 0x7fffffffu) + (YOND_NUDGE_ULPS);
    if (m < 0) m = 0;
    if (m > 0x7f7fffff) m = 0x7f7fffff;
    b = (b & 0x80000000u) | (uint32_t)m;
    memcpy(&x, &b, 4);
    return x;
}
static inline float yond_nudged_logf(float x) { return yond_nudge(logf(x)); }
static inline float yond_nudged_expf(float x) { return yond_nudge(expf(x)); }
static inline float yond_nudged_log1pf(float x) { return yond_nudge(log1pf(x)); }
static inline float yond_nudged_expm1f(float x) { return yond_nudge(expm1f(x)); }
#define logf yond_nudged_logf
#define expf yond_nudged_expf
#define log1pf yond_nudged_log1pf
#define expm1f yond_nudged_expm1f
#endif

#include "../yond_public_amd/csrc/pgnoise_sampler.h"

// the raw words of philox.h (the file the kernels compile) for n counters and keys: out[4 i .. 4 i + 3]
extern "C" void yond_host_philox(size_t n, const uint32_t* c0, const uint32_t* c1, const uint32_t* c2, const uint32_t* c3, const uint32_t* k0,
                                 const uint32_t* k1, uint32_t* out) {
    for (size_t i = 0; i < n; ++i) {
        const Philox4 r = philox4x32_10(c0[i], c1[i], c2[i], c3[i], k0[i], k1[i]);
        for (int j = 0; j < 4; ++j) out[4 * i + j] = r.v[j];
    }
}

extern "C" void pg_host_draw(unsigned key, unsigned slot, unsigned long long first, size_t n, const float* lam, size_t n_lam, float* k,
                             float* z) {
    for (size_t i = 0; i < n; ++i) {
        const PGDraw d = pg_draw(key, slot, first + i, lam[i % n_lam]);
        k[i] = d.k;
        z[i] = d.z;
    }
}
