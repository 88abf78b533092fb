// I1: sRGB crops -> raw training pairs (data_process/unprocess.py:80-148 + yond_datasets.py:15-19, 277-334), one launch per batch.
// House rules: asynchronous on the caller's stream, no allocation or synchronisation in the launch function, 16-byte stores,
// no scratch.  One thread = one group of 4 consecutive output elements of a patch ([c][y][x] order), so hr / lr leave as float4
// and one Philox4x32-10 call gives the group's 4 normals.  Each element gathers one source pixel (the rotation and the mosaic are
// index maps), looks its 3 levels up in the transfer curve (LDS for uint8, L2-resident global memory for uint16), applies the CCM
// and the gain mask and keeps the one channel its mosaic site needs.  grid = (ceil(h'w' / 256), B).
#include "common.h"
#include "philox.h"

#define I2R_T 256

template <typename T>
__global__ __launch_bounds__(I2R_T) void img2raw_kernel(const T* __restrict__ crops, size_t crops_len, int H, int W,
                                                        const float* __restrict__ curve, const YondImg2RawPatch* __restrict__ patches,
                                                        int pattern, int clip, float* __restrict__ hr, float* __restrict__ lr,
                                                        float* __restrict__ sigma_out) {
    constexpr bool kLds = sizeof(T) == 1;
    __shared__ float s_curve[kLds ? 256 : 1];
    const int b = blockIdx.y;
    const YondImg2RawPatch& p = patches[b];
    if (kLds) {
        s_curve[threadIdx.x] = curve[threadIdx.x];
        __syncthreads();
    }
    const int k = pattern >= 0 ? pattern : (p.pattern & 3);
    const int ho = (k & 1) ? W / 2 : H / 2, wo = (k & 1) ? H / 2 : W / 2;
    const int plane = ho * wo;
    const int q = blockIdx.x * I2R_T + threadIdx.x;           // 4-element group; a patch has 4 * plane elements = plane groups
    if (q >= plane) return;
    if (q == 0 && sigma_out) sigma_out[b] = p.sigma;
    f32x4* hr4 = reinterpret_cast<f32x4*>(hr + (size_t)b * 4 * plane) + q;
    f32x4* lr4 = reinterpret_cast<f32x4*>(lr + (size_t)b * 4 * plane) + q;
    const size_t npix = (size_t)H * W * 3;
    if (p.offset < 0 || (size_t)p.offset > crops_len || crops_len - (size_t)p.offset < npix) {
        const float nan = __builtin_nanf("");
        *hr4 = f32x4{nan, nan, nan, nan};
        *lr4 = f32x4{nan, nan, nan, nan};
        return;
    }
    const T* img = crops + p.offset;
    float m[9], g[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) m[i] = p.rgb2cam[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) g[i] = p.gain[i];
    const float sigma = p.sigma;

    // (c, y, x) of the group's first element, then stepped
    int e = 4 * q;
    int c = e / plane, r = e - c * plane;
    int y = r / wo, x = r - y * wo;
    float out[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int i = 2 * y + (c >> 1), j = 2 * x + (c & 1);   // site in the rotated full mosaic
        int Y, X;                                               // np.rot90(bayer, k): source site
        if (k == 0) { Y = i; X = j; }
        else if (k == 1) { Y = j; X = W - 1 - i; }
        else if (k == 2) { Y = H - 1 - i; X = W - 1 - j; }
        else { Y = H - 1 - j; X = i; }
        const int ch = (Y & 1) + (X & 1);                       // RGGB: R at (0,0), G at (0,1) and (1,0), B at (1,1)
        const T* px = img + ((size_t)Y * W + X) * 3;
        float v[3];
#pragma unroll
        for (int t = 0; t < 3; ++t) v[t] = kLds ? s_curve[px[t]] : curve[px[t]];
        float cam[3];
#pragma unroll
        for (int t = 0; t < 3; ++t) cam[t] = v[0] * m[3 * t] + v[1] * m[3 * t + 1] + v[2] * m[3 * t + 2];
        const float gray = (cam[0] + cam[1] + cam[2]) / 3.0f;
        float mask = fmaxf(gray - 0.9f, 0.0f) / 0.1f;
        mask = mask * mask;
        const float gc = ch == 0 ? g[0] : (ch == 1 ? g[1] : g[2]);
        const float cc = ch == 0 ? cam[0] : (ch == 1 ? cam[1] : cam[2]);
        const float o = cc * fmaxf(mask + (1.0f - mask) * gc, gc);
        out[u] = fminf(fmaxf(o, 0.0f), 1.0f);
        if (++x == wo) {
            x = 0;
            if (++y == ho) { y = 0; ++c; }
        }
    }
    const Philox4 rnd = philox4x32_10((uint32_t)q, 0u, 0u, 0u, p.key, p.slot);
    float z[4];
    box_muller(rnd.v[0], rnd.v[1], z[0], z[1]);
    box_muller(rnd.v[2], rnd.v[3], z[2], z[3]);
    f32x4 h4, l4;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        float l = out[u] + z[u] * sigma;
        if (clip) l = fminf(fmaxf(l, 0.0f), 1.0f);
        h4[u] = out[u];
        l4[u] = l;
    }
    *hr4 = h4;
    *lr4 = l4;
}

extern "C" int yond_img2raw_f32(const void* crops, size_t crops_len, int dtype, int H, int W, const float* curve,
                                const YondImg2RawPatch* patches, int B, int pattern, int clip, float* hr, float* lr, float* sigma,
                                void* stream) {
    if (!crops || !curve || !patches || !hr || !lr) return YOND_EINVAL;
    if (H < 2 || W < 2 || (H & 1) || (W & 1) || B < 1 || (dtype != 0 && dtype != 1)) return YOND_EINVAL;
    if (pattern < -1 || pattern > 3 || (pattern == -1 && H != W)) return YOND_EINVAL;
    const int plane = (H / 2) * (W / 2);
    const dim3 grid((plane + I2R_T - 1) / I2R_T, B);
    if (dtype == 0)
        hipLaunchKernelGGL(img2raw_kernel<uint8_t>, grid, dim3(I2R_T), 0, (hipStream_t)stream, (const uint8_t*)crops, crops_len, H, W,
                           curve, patches, pattern, clip, hr, lr, sigma);
    else
        hipLaunchKernelGGL(img2raw_kernel<uint16_t>, grid, dim3(I2R_T), 0, (hipStream_t)stream, (const uint16_t*)crops, crops_len, H,
                           W, curve, patches, pattern, clip, hr, lr, sigma);
    YOND_LAUNCH_CHECK();
    return YOND_OK;
}
