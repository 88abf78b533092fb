// The sampler of csrc/pgnoise_sampler.h compiled for the CPU (tests/test_pgnoise_host.py test_sampler_on_the_cpu): the same source the kernel runs,
// with the host C library's logf / expf / sinf / cosf in place of the device's.
#include <stddef.h>

#include "../yond_public_amd/csrc/pgnoise_sampler.h"

extern "C" void pg_host_draw(unsigned key, unsigned slot, unsigned long long first, size_t n, const float* lam, size_t n_lam, float* k,
                             float* z) {
    for (size_t i = 0; i < n; ++i) {
        const PGDraw d = pg_draw(key, slot, first + i, lam[i % n_lam]);
        k[i] = d.k;
        z[i] = d.z;
    }
}
