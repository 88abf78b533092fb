// I3: camera noise on clean frames or batches (data_process/process.py:631-671 generate_noisy_obs): Poisson or Gaussian-approximated shot
// noise, Tukey-lambda or Gaussian read noise, row noise, quantisation noise and a per-channel dark bias, one launch per batch.  The
// contract is in include/yond_hip.h.  House rules and launch shape as pgnoise.hip: asynchronous on the caller's stream, no allocation or
// synchronisation in the launch function, each item cut at the 16-byte boundaries of its OUTPUT (up to 3 head elements, float4 groups,
// up to 3 tail elements), 16-byte loads and stores, no LDS, no scratch, no device printf / assert.  In place is safe: a thread reads the
// elements it writes before it writes them and nobody else touches them.
// An element's value is a function of (its item, its index in the item, its clean value, the geometry): camnoise_sampler.h draws from
// Philox4x32-10 with the element index (or the row index) in the counter.  The terms are summed in the order of pgnoise.hip's
// pg_element and each is divided by the exposure on its own, so an item with only Poisson shot and Gaussian read noise is that kernel's
// output bit for bit; the clip to [clip_lo, clip_hi] before the division by e is applied as a clip to [clip_lo / e, clip_hi / e] after
// it (the same set of values: float division by e > 0 is monotonic).
// What an item does not use it does not pay for: the element draw is skipped when the item has neither Tukey-lambda read noise nor
// quantisation nor the Gaussian shot approximation, the row draw when sig_row is 0, and the row draw is made once per run of elements
// in one row (a float4 group crosses a row boundary at most once for row_len >= 4).
// grid = (min(ceil(groups / 256), CAM_MAX_BLOCKS), B), grid-stride over the groups of one item.
#include "common.h"
#include "camnoise_sampler.h"

#define CAM_T 256
#define CAM_MAX_BLOCKS (1 << 20)
#define CAM_FLT_MAX 3.402823466e38f

// what is the same for every element of an item (wave-uniform: scalar registers).  The switches are bits of one word, tested where they
// are used: a bool apiece would hold a 64-bit lane mask each across the sampler.
#define CAM_F_DRAW 8u       /* the element draw is needed */
#define CAM_F_EXTRA 16u     /* row, quantisation or bias term present */
#define CAM_F_GEOM 32u      /* row or bias term present and a geometry given */
#define CAM_F_ROW 64u       /* row term present and a geometry given */
struct CamItemCtx {
    float sr, srow;         // sig_read / mfm, sig_row / mfm
    float lo, hi;           // clip_lo / e, clip_hi / e
    uint32_t f;             // YOND_CAM_* of the item's flags | CAM_F_*
};

__device__ __forceinline__ CamItemCtx cam_ctx(const YondCamItem& it, int row_len) {
    CamItemCtx c;
    c.sr = it.sig_read / it.mfm;
    c.srow = it.sig_row / it.mfm;
    c.lo = it.clip_lo / it.exposure;
    c.hi = it.clip_hi / it.exposure;
    c.f = it.flags & (YOND_CAM_POISSON | YOND_CAM_TUKEY | YOND_CAM_CLIP);
    const bool bias = it.bias[0] != 0.0f || it.bias[1] != 0.0f || it.bias[2] != 0.0f || it.bias[3] != 0.0f;
    const bool rown = it.sig_row != 0.0f;
    if ((c.f & YOND_CAM_TUKEY) || it.q_step != 0.0f || (!(c.f & YOND_CAM_POISSON) && it.beta1 > 0.0f)) c.f |= CAM_F_DRAW;
    if (bias || rown || it.q_step != 0.0f) c.f |= CAM_F_EXTRA;
    if ((bias || rown) && row_len > 0) c.f |= CAM_F_GEOM;
    if (rown && row_len > 0) c.f |= CAM_F_ROW;
    return c;
}

// zrow: the row's normal (0 where the item has no row noise), ch: the element's CFA channel
__device__ __forceinline__ float cam_element(const YondCamItem& it, const CamItemCtx& c, uint64_t index, float x, float zrow, int ch) {
    if (!(fabsf(x) <= CAM_FLT_MAX)) return __builtin_nanf("");            // NaN, +-inf
    const float e = it.exposure, beta1 = it.beta1, m = it.mfm;
    const float xp = fmaxf(x, 0.0f);
    const bool shot = beta1 > 0.0f;
    const float y = xp * e;
    float lam = shot ? m * y / beta1 : 0.0f;
    const bool huge = !(lam <= CAM_FLT_MAX);                                // overflowed: the count is not representable, its relative noise is nil
    if (huge || !(c.f & YOND_CAM_POISSON)) lam = 0.0f;
    const PGDraw d = pg_draw(it.key, it.slot, index, lam);
    CamDraw cd = {0.0f, 0.0f, 0.0f};
    if (c.f & CAM_F_DRAW) cd = cam_draw(it.key, it.slot, index, it.lam);
    float signal = xp;                                                      // already / e
    if (shot && !huge) {
        if (c.f & YOND_CAM_POISSON) signal = ((d.k * beta1) / m) / e;
        else signal = (y + cd.zs * sqrtf(fmaxf(y / beta1, 1e-10f)) * beta1 / m) / e;
    }
    const float read = c.sr * ((c.f & YOND_CAM_TUKEY) ? cd.tl : d.z);
    float v = signal + fminf(x, 0.0f) + read / e;
    if (c.f & CAM_F_EXTRA) {
        const float b = ch == 0 ? it.bias[0] : (ch == 1 ? it.bias[1] : (ch == 2 ? it.bias[2] : it.bias[3]));    // selects: no scratch
        v += (c.srow * zrow + it.q_step * cd.uq + b) / e;
    }
    v = fminf(fmaxf(v, -CAM_FLT_MAX), CAM_FLT_MAX);                         // a finite x never gives an infinity or a NaN
    if (c.f & YOND_CAM_CLIP) v = fminf(fmaxf(v, c.lo), c.hi);
    return v;
}

// clean and noisy carry no __restrict__: they may be the same pointer
__global__ __launch_bounds__(CAM_T) void cam_noise_kernel(const float* clean, float* noisy, size_t n, const YondCamItem* __restrict__ items,
                                                          int layout, int row_len) {
    const int b = blockIdx.y;
    const YondCamItem it = items[b];
    const CamItemCtx c = cam_ctx(it, row_len);
    const size_t base = (size_t)b * n;
    const float* src = clean + base;
    float* dst = noisy + base;
    size_t head = (size_t)((16u - (unsigned)((uintptr_t)dst & 15u)) & 15u) >> 2;
    if (head > n) head = n;
    const size_t groups = (n - head) >> 2;
    const size_t tail0 = head + 4 * groups;                                // first tail element; n - tail0 <= 3
    const bool src_aligned = (((uintptr_t)(src + head)) & 15u) == 0;
    const size_t stride = (size_t)gridDim.x * CAM_T;
    const size_t plane = n >> 2;                                           // layout 0: elements per channel
    // work units: [0, groups) the float4 groups, then the head [0, head) and the tail [tail0, n) as units of up to 3 elements
    for (size_t g = (size_t)blockIdx.x * CAM_T + threadIdx.x; g < groups + 2; g += stride) {
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
        // geometry of the unit's first element; the loop below steps it.  Without one (row_len 0) the item is one row of channel 0.
        uint32_t row = 0, col = 0;                                         // (a geometry comes with n < 2^32: 32-bit division)
        if (c.f & CAM_F_GEOM) {
            row = (uint32_t)i0 / (uint32_t)row_len;
            col = (uint32_t)i0 - row * (uint32_t)row_len;
        }
        uint32_t zrow_of = ~0u;
        float zrow = 0.0f;
        f32x4 y = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 1
        for (int u = 0; u < 4; ++u) {                                      // one copy of the sampler: x and y rotate through lanes 0 / 3
            float r = 0.0f;
            if (u < cnt) {
                const uint64_t i = (uint64_t)(i0 + u);
                int ch = 0;
                if (c.f & CAM_F_GEOM) {
                    if (layout == 0) ch = (int)(i >= plane) + (int)(i >= 2 * plane) + (int)(i >= 3 * plane);
                    else ch = 2 * (int)(row & 1u) + (int)(col & 1u);
                    if ((c.f & CAM_F_ROW) && row != zrow_of) {
                        zrow = cam_row_normal(it.key, it.slot, row);
                        zrow_of = row;
                    }
                }
                r = cam_element(it, c, i, x[0], zrow, ch);
                if (++col == (uint32_t)row_len) {
                    col = 0;
                    ++row;
                }
            }
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

extern "C" int yond_camera_noise_f32(const float* clean, float* noisy, size_t n_per_item, int B, const YondCamItem* items, int layout,
                                     int row_len, void* stream) {
    if (!clean || !noisy || !items) return YOND_EINVAL;
    if (B < 1 || B > 65535 || n_per_item == 0) return YOND_EINVAL;
    if ((((uintptr_t)clean) | ((uintptr_t)noisy)) & 3u) return YOND_EINVAL;
    if ((layout != 0 && layout != 1) || row_len < 0) return YOND_EINVAL;
    if (row_len > 0) {
        if (n_per_item > 0xffffffffull) return YOND_EINVAL;
        if (layout == 0 && ((n_per_item & 3u) || (n_per_item >> 2) % (size_t)row_len)) return YOND_EINVAL;
        if (layout == 1 && n_per_item % (size_t)row_len) return YOND_EINVAL;
    }
    const size_t groups = n_per_item / 4 + 2;                    // float4 groups + the head and tail units
    size_t blocks = (groups + CAM_T - 1) / CAM_T;
    if (blocks > CAM_MAX_BLOCKS) blocks = CAM_MAX_BLOCKS;
    hipLaunchKernelGGL(cam_noise_kernel, dim3((unsigned)blocks, (unsigned)B), dim3(CAM_T), 0, (hipStream_t)stream, clean, noisy,
                       n_per_item, items, layout, row_len);
    YOND_LAUNCH_CHECK();
    return YOND_OK;
}
