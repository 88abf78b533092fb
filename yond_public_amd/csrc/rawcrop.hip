// I4: whole clean raw frames -> raw training pairs (data_process/yond_datasets.py:153-212, SID_Raw_Dataset.__getitem__), one launch
// per batch of up to RC_CHUNK patches.  House rules: asynchronous on the caller's stream, no allocation or synchronisation in the
// launch function, 16-byte stores, no scratch.  One thread = one group of 4 consecutive output elements of a patch ([c][y][x]
// order), so hr / lr leave as float4 and one Philox4x32-10 call gives the group's 4 normals.  Each element gathers one Bayer pixel
// of the resident frame (the rotation, the packing and the crop are index maps) and takes it through the reference's float32 steps,
// every one rounded once (rounding intrinsics, a correctly rounded sqrtf, -ffp-contract=off).  The patch descriptors are read and checked on the HOST (a crop outside its frame never
// reaches the device) and travel to the kernel by value in its argument block: nothing of the caller's array is read after the
// export returns.  grid = (ceil(ps * ps / 256), patches of the chunk).
#include "common.h"
#include "philox.h"

#define RC_T 256
#define RC_CHUNK 64

struct RcPatch {              // YondRawCropPatch as the kernel takes it: 56 bytes
    long long frame;
    double gain0, gain2;
    int y0, x0;
    int pattern_vst;          // pattern | vst_aug << 2
    float rgb_gain, sigma;
    unsigned key, slot;
    int pad_;
};
struct RcArgs {
    RcPatch p[RC_CHUNK];
};
static_assert(sizeof(RcPatch) == 56, "RcPatch layout");
static_assert(sizeof(RcArgs) + 128 <= 3840, "the kernel's argument block (with the launch's hidden arguments) must stay below 4 KiB");

__device__ __forceinline__ float rc_dn(const uint16_t* f, long long i) { return (float)f[i]; }
__device__ __forceinline__ float rc_dn(const float* f, long long i) { return f[i]; }

template <typename T>
__global__ __launch_bounds__(RC_T) void rawcrop_kernel(const T* __restrict__ frames, int H, int W, float bl, float den, int ps, int clip,
                                                       int b0, float* __restrict__ hr, float* __restrict__ lr,
                                                       float* __restrict__ sigma_out, const RcArgs args) {
    const RcPatch& p = args.p[blockIdx.y];
    const int plane = ps * ps;                                  // a patch has 4 * plane elements = plane groups of 4
    const int q = blockIdx.x * RC_T + threadIdx.x;
    if (q >= plane) return;
    const int b = b0 + blockIdx.y;
    if (q == 0 && sigma_out) sigma_out[b] = p.sigma;
    const T* img = frames + p.frame;
    const int k = p.pattern_vst & 3, vst = p.pattern_vst >> 2;
    const float rgb_gain = p.rgb_gain, sigma = p.sigma;
    const double g0 = p.gain0, g2 = p.gain2;

    // (c, y, x) of the group's first element, then stepped
    int e = 4 * q;
    int c = e / plane, r = e - c * plane;
    int y = r / ps, x = r - y * ps;
    float out[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int i = 2 * (p.y0 + y) + (c >> 1), j = 2 * (p.x0 + x) + (c & 1);   // site in the rotated Bayer frame
        int Y, X;                                                                 // np.rot90(bayer, k): source site
        if (k == 0) { Y = i; X = j; }
        else if (k == 1) { Y = j; X = W - 1 - i; }
        else if (k == 2) { Y = H - 1 - i; X = W - 1 - j; }
        else { Y = H - 1 - j; X = i; }
        float v = __fdiv_rn(__fsub_rn(rc_dn(img, (long long)Y * W + X), bl), den);
        v = fminf(fmaxf(v, 0.0f), 1.0f);
        // sqrtf, not __fsqrt_rn: the HIP headers map that name to the approximate native square root (measured 1-2 ulp off
        // NumPy's); sqrtf is correctly rounded under hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt
        if (vst) v = sqrtf(v);
        v = __fmul_rn(v, rgb_gain);
        if (c == 0) v = __double2float_rn(__dmul_rn((double)v, g0));
        else if (c == 2) v = __double2float_rn(__dmul_rn((double)v, g2));
        out[u] = v;
        if (++x == ps) {
            x = 0;
            if (++y == ps) { y = 0; ++c; }
        }
    }
    const Philox4 rnd = philox4x32_10((uint32_t)q, 0u, 0u, 0u, p.key, p.slot);
    float z[4];
    box_muller(rnd.v[0], rnd.v[1], z[0], z[1]);
    box_muller(rnd.v[2], rnd.v[3], z[2], z[3]);
    f32x4 h4, l4;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        float h = out[u];
        float l = __fadd_rn(h, __fmul_rn(z[u], sigma));
        if (clip) {
            h = fminf(fmaxf(h, 0.0f), 1.0f);
            l = fminf(fmaxf(l, 0.0f), 1.0f);
        }
        h4[u] = h;
        l4[u] = l;
    }
    const size_t o = ((size_t)b * plane + q) * 4;
    if ((((uintptr_t)hr | (uintptr_t)lr) & 15) == 0) {          // uniform: the buffers' own alignment decides the store width
        *reinterpret_cast<f32x4*>(hr + o) = h4;
        *reinterpret_cast<f32x4*>(lr + o) = l4;
    } else {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            hr[o + u] = h4[u];
            lr[o + u] = l4[u];
        }
    }
}

extern "C" int yond_rawcrop_f32(const void* frames, size_t frames_len, int dtype, int H, int W, float bl, float wp,
                                const YondRawCropPatch* patches, int B, int ps, int clip, float* hr, float* lr, float* sigma,
                                void* stream) {
    if (!frames || !patches || !hr || !lr || !sigma) return YOND_EINVAL;
    if (H < 2 || W < 2 || (H & 1) || (W & 1) || B < 1 || ps < 1 || (dtype != 0 && dtype != 1)) return YOND_EINVAL;
    if (ps > 16384 || !(wp > bl)) return YOND_EINVAL;            // ps * ps groups are counted in an int
    const size_t npix = (size_t)H * W;
    for (int b = 0; b < B; ++b) {                                // every patch is checked before the first launch
        const YondRawCropPatch& p = patches[b];
        if (p.pattern < 0 || p.pattern > 3 || (p.vst_aug != 0 && p.vst_aug != 1)) return YOND_EINVAL;
        const int ho = ((p.pattern & 1) ? W : H) / 2, wo = ((p.pattern & 1) ? H : W) / 2;
        if (p.y0 < 0 || p.x0 < 0 || p.y0 > ho - ps || p.x0 > wo - ps) return YOND_EINVAL;
        if (p.frame < 0 || (size_t)p.frame > frames_len || frames_len - (size_t)p.frame < npix) return YOND_EINVAL;
    }
    const float den = wp - bl;
    const int plane = ps * ps;
    for (int b0 = 0; b0 < B; b0 += RC_CHUNK) {
        const int nb = B - b0 < RC_CHUNK ? B - b0 : RC_CHUNK;
        RcArgs args;
        for (int i = 0; i < RC_CHUNK; ++i) {
            const YondRawCropPatch& p = patches[b0 + (i < nb ? i : 0)];
            args.p[i] = RcPatch{p.frame, p.gain0, p.gain2, p.y0, p.x0, p.pattern | (p.vst_aug << 2), p.rgb_gain, p.sigma, p.key, p.slot, 0};
        }
        const dim3 grid((plane + RC_T - 1) / RC_T, nb);
        if (dtype == 0)
            hipLaunchKernelGGL(rawcrop_kernel<uint16_t>, grid, dim3(RC_T), 0, (hipStream_t)stream, (const uint16_t*)frames, H, W, bl, den,
                               ps, clip, b0, hr, lr, sigma, args);
        else
            hipLaunchKernelGGL(rawcrop_kernel<float>, grid, dim3(RC_T), 0, (hipStream_t)stream, (const float*)frames, H, W, bl, den, ps,
                               clip, b0, hr, lr, sigma, args);
        YOND_LAUNCH_CHECK();
    }
    return YOND_OK;
}
