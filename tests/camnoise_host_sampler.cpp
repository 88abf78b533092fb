// The sampler of csrc/camnoise_sampler.h compiled for the CPU (tests/test_camnoise_host.py): the same source the kernel runs, with the host
// C library's logf / log1pf / expm1f / sinf / cosf in place of the device's.  As a shared library it hands the draws to the tests; with
// -DCAMNOISE_HOST_MAIN it is a stand-alone program (for a sanitizer build) that walks every shape of the tests, the index range across
// 2^32 and hostile shapes, and fails on a non-finite draw.
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

#include "../yond_public_amd/csrc/camnoise_sampler.h"

// the raw words of philox.h (the file the kernels compile) for n counters and keys: out[4 i .. 4 i + 3]
extern "C" void yond_host_philox(size_t n, const uint32_t* c0, const uint32_t* c1, const uint32_t* c2, const uint32_t* c3, const uint32_t* k0,
                                 const uint32_t* k1, uint32_t* out) {
    for (size_t i = 0; i < n; ++i) {
        const Philox4 r = philox4x32_10(c0[i], c1[i], c2[i], c3[i], k0[i], k1[i]);
        for (int j = 0; j < 4; ++j) out[4 * i + j] = r.v[j];
    }
}

extern "C" void cam_host_draw(unsigned key, unsigned slot, unsigned long long first, size_t n, float lam, float* tl, float* uq, float* zs) {
    for (size_t i = 0; i < n; ++i) {
        const CamDraw d = cam_draw(key, slot, first + i, lam);
        tl[i] = d.tl;
        uq[i] = d.uq;
        zs[i] = d.zs;
    }
}

extern "C" void cam_host_rows(unsigned key, unsigned slot, unsigned long long first_row, size_t n, float* z) {
    for (size_t i = 0; i < n; ++i) z[i] = cam_row_normal(key, slot, first_row + i);
}

// Q_lam at the uniform's two ends
extern "C" void cam_host_tail(float lam, float* q) {
    q[0] = cam_tl_quantile(lam, 1.16415321826934814453125e-10f);
    q[1] = cam_tl_quantile(lam, 0.5f);
}

#ifdef CAMNOISE_HOST_MAIN
#include <stdio.h>
#include <vector>

int main() {
    const float lams[] = {-0.26f, -0.026f, 0.0f, 0.015f, 0.102f, -0.49f, 1e-30f, -1e-30f, 5.0f, -5.0f, 1e30f, -1e30f};
    const unsigned long long firsts[] = {0ull, 0xfffffff0ull, 0xfffffffffffffff0ull};
    const size_t n = 4096;
    std::vector<float> tl(n), uq(n), zs(n), z(n);
    double sum = 0.0;
    int bad = 0;
    for (float lam : lams) {
        for (unsigned long long first : firsts) {
            cam_host_draw(20261019u, 3u, first, n, lam, tl.data(), uq.data(), zs.data());
            cam_host_rows(20261019u, 3u, first, n, z.data());
            for (size_t i = 0; i < n; ++i) {
                if (!(fabsf(tl[i]) <= 3.402823466e38f) || !(fabsf(uq[i]) < 0.5f) || !(fabsf(zs[i]) < 6.0f) || !(fabsf(z[i]) < 6.0f)) ++bad;
                sum += (fabsf(tl[i]) < 1e30f ? tl[i] : 0.0) + uq[i] + zs[i] + z[i];
            }
        }
        float q[2];
        cam_host_tail(lam, q);
        printf("lam %g: Q(2^-33) = %g, Q(1/2) = %g\n", lam, q[0], q[1]);
    }
    printf("checksum %.6f, %d bad draws\n", sum, bad);
    return bad ? 1 : 0;
}
#endif
