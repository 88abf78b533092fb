// I2: Poisson-Gaussian noise on clean frames or batches (data_process/yond_datasets.py:720, the method's noise model), one launch
// per batch.  House rules as in img2raw.hip: asynchronous on the caller's stream, no allocation or synchronisation in the launch
// function, 16-byte loads and stores, no scratch, no device printf / assert.
// An element's value is a function of (its item's parameters, its index in the item, its clean value): pgnoise_sampler.h draws from
// Philox4x32-10 with the 64-bit element index in the counter, so the launch geometry and the pointers' alignment decide only which
// thread computes an element.  Each item is cut at the 16-byte boundaries of its OUTPUT: up to 3 head elements, float4 groups, up to
// 3 tail elements; the groups are loaded as float4 when `clean` shares the alignment and as four scalars otherwise.  In place is
// safe: a thread reads the elements it writes before it writes them and nobody else touches them.
// grid = (min(ceil(groups / 256), PG_MAX_BLOCKS), B), grid-stride over the groups of one item.
#include "common.h"
#include "pgnoise_element.h"

#define PG_T 256
#define PG_MAX_BLOCKS (1 << 20)

// clean and noisy carry no __restrict__: they may be the same pointer
__global__ __launch_bounds__(PG_T) void pg_noise_kernel(const float* clean, float* noisy, size_t n, const YondPGItem* __restrict__ items,
                                                        int clip) {
    const int b = blockIdx.y;
    const YondPGItem it = items[b];
    const size_t base = (size_t)b * n;
    const float* src = clean + base;
    float* dst = noisy + base;
    size_t head = (size_t)((16u - (unsigned)((uintptr_t)dst & 15u)) & 15u) >> 2;
    if (head > n) head = n;
    const size_t groups = (n - head) >> 2;
    const size_t tail0 = head + 4 * groups;                                // first tail element; n - tail0 <= 3
    const bool src_aligned = (((uintptr_t)(src + head)) & 15u) == 0;
    const size_t stride = (size_t)gridDim.x * PG_T;
    // work units: [0, groups) the float4 groups, then the head [0, head) and the tail [tail0, n) as units of up to 3 elements
    for (size_t g = (size_t)blockIdx.x * PG_T + threadIdx.x; g < groups + 2; g += stride) {
        const bool full = g < groups;
        const size_t i0 = full ? head + 4 * g : (g == groups ? 0 : tail0);
        const int cnt = full ? 4 : (g == groups ? (int)head : (int)(n - tail0));
        f32x4 x = {0.0f, 0.0f, 0.0f, 0.0f};
        if (full && src_aligned) {
            x = *reinterpret_cast<const f32x4*>(src + i0);
        } else {
            if (cnt > 0) x[0] = src[i0];
            if (cnt > 1) x[1] = src[i0 + 1];
            if (cnt > 2) x[2] = src[i0 + 2];
            if (cnt > 3) x[3] = src[i0 + 3];
        }
        f32x4 y = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 1
        for (int u = 0; u < 4; ++u) {                                      // one copy of the sampler: x and y rotate through lanes 0 / 3
            const float r = u < cnt ? pg_element(it, (uint64_t)(i0 + u), x[0], clip) : 0.0f;
            x = f32x4{x[1], x[2], x[3], x[0]};
            y = f32x4{y[1], y[2], y[3], r};
        }
        if (full) {
            *reinterpret_cast<f32x4*>(dst + i0) = y;
        } else {
            if (cnt > 0) dst[i0] = y[0];
            if (cnt > 1) dst[i0 + 1] = y[1];
            if (cnt > 2) dst[i0 + 2] = y[2];
        }
    }
}

extern "C" int yond_pg_noise_f32(const float* clean, float* noisy, size_t n_per_item, int B, const YondPGItem* items, int clip,
                                 void* stream) {
    if (!clean || !noisy || !items) return YOND_EINVAL;
    if (B < 1 || B > 65535 || n_per_item == 0 || (clip != 0 && clip != 1)) return YOND_EINVAL;
    if ((((uintptr_t)clean) | ((uintptr_t)noisy)) & 3u) return YOND_EINVAL;
    const size_t groups = n_per_item / 4 + 2;                    // float4 groups + the head and tail units
    size_t blocks = (groups + PG_T - 1) / PG_T;
    if (blocks > PG_MAX_BLOCKS) blocks = PG_MAX_BLOCKS;
    hipLaunchKernelGGL(pg_noise_kernel, dim3((unsigned)blocks, (unsigned)B), dim3(PG_T), 0, (hipStream_t)stream, clean, noisy,
                       n_per_item, items, clip);
    YOND_LAUNCH_CHECK();
    return YOND_OK;
}
