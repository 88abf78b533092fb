// The sampler of csrc/camnoise_sampler.h compiled for the CPU (tests/test_camnoise_host.py): the same source the kernel runs, with the host
// C library's logf / log1pf / expm1f / sinf / cosf in place of the device's.  As a shared library it hands the draws to the tests; with
// -DCAMNOISE_HOST_MAIN it is a stand-alone program (for a sanitizer build) that walks every shape of the tests, the index range across
// 2^32 and hostile shapes, and fails on a non-finite draw.
#include <stddef.h>

#include "../yond_public_amd/csrc/camnoise_sampler.h"

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
