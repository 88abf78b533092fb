// Edge layers of the noise-estimation network EstUnet (archs/Unet.py:474-611): the first 3x3 convolution on one
// full-resolution Bayer plane and the 1x1 head with its optional square and spatial mean.  Everything between them runs
// on the denoiser's convolution, pooling and decoder-GEMM launches (engine.py / estnet.py).
#include "common.h"

// ------------------------------------------------------------------------------------------------------
// E1  first layer: 3x3, Cin = 1, zero padding 1, + bias, ReLU, stored [N][H][W][Cout].  HBM bound: 4 B in, 4*Cout B out
// per pixel.  A workgroup takes an 8 x 64 pixel tile; its input (10 x 66 values) goes through LDS once.  Lane group
// G = Cout/4 lanes per pixel, each lane holds the 9 x 4 weights of its four channels in registers and stores 16 bytes:
// a wave writes 64 x 16 contiguous bytes.
// ------------------------------------------------------------------------------------------------------
constexpr int EST_TH = 8, EST_TW = 64;

__global__ __launch_bounds__(256) void est_conv_in_kernel(const float* __restrict__ x, int H, int W, int Cout,
                                                          const float* __restrict__ w, const float* __restrict__ bias,
                                                          float* __restrict__ dst) {
    __shared__ float s_in[(EST_TH + 2) * (EST_TW + 2)];
    const int tid = threadIdx.x;
    const int ntx = (W + EST_TW - 1) / EST_TW;
    const int tx = blockIdx.x % ntx, ty = blockIdx.x / ntx;
    const int n = blockIdx.y;
    const int ox0 = tx * EST_TW, oy0 = ty * EST_TH;
    const float* xn = x + (size_t)n * H * W;
    for (int it = tid; it < (EST_TH + 2) * (EST_TW + 2); it += 256) {
        const int py = it / (EST_TW + 2), px = it - py * (EST_TW + 2);
        const int gy = oy0 - 1 + py, gx = ox0 - 1 + px;
        s_in[it] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? xn[(size_t)gy * W + gx] : 0.0f;
    }
    const int G = Cout / 4;
    const int npix = 256 / G;
    const int cg = tid % G, pix = tid / G;
    f32x4 wr[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) wr[t][e] = w[(4 * cg + e) * 9 + t];
    const f32x4 b = *(const f32x4*)(bias + 4 * cg);
    __syncthreads();
    if (pix >= npix) return;
    for (int q = pix; q < EST_TH * EST_TW; q += npix) {
        const int r = q / EST_TW, c = q - r * EST_TW;
        const int oy = oy0 + r, ox = ox0 + c;
        if (oy >= H || ox >= W) continue;
        f32x4 acc = b;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const float v = s_in[(r + t / 3) * (EST_TW + 2) + c + t % 3];
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = fmaf(wr[t][e], v, acc[e]);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = fmaxf(acc[e], 0.0f);
        *(f32x4*)(dst + (((size_t)n * H + oy) * W + ox) * Cout + 4 * cg) = acc;
    }
}

extern "C" int yond_est_conv_in_f32(const float* x, int N, int H, int W, int Cout, const float* w, const float* bias, float* dst,
                                    void* stream) {
    if (!x || !w || !bias || !dst || N <= 0 || H <= 0 || W <= 0 || N > 65535) return YOND_EINVAL;
    if (Cout <= 0 || Cout % 32 != 0 || Cout > 1024) return YOND_EUNSUPPORTED;
    const long long tiles = (long long)((W + EST_TW - 1) / EST_TW) * ((H + EST_TH - 1) / EST_TH);
    if (tiles > 0x7fffffffLL) return YOND_EUNSUPPORTED;
    hipLaunchKernelGGL(est_conv_in_kernel, dim3((unsigned)tiles, N), dim3(256), 0, (hipStream_t)stream, x, H, W, Cout, w, bias, dst);
    YOND_LAUNCH_CHECK();
    return YOND_OK;
}

// ------------------------------------------------------------------------------------------------------
// E2  head: 1x1 Cin -> out_nc (<= 4) + bias, optionally squared ('var'); either the map [N][out_nc][H][W] or the spatial mean
// [N][out_nc].  16 lanes per pixel read its Cin channels as 16-byte loads (a wave reads 4 pixels = 4*Cin*4 contiguous bytes)
// and reduce by shuffles.  The mean is deterministic: each workgroup of an image sums a fixed, strided set of pixel groups in
// float64 in a fixed order and writes one partial per channel; a second launch adds an image's partials in a fixed order.
// ------------------------------------------------------------------------------------------------------
constexpr int EST_LPP = 16;                    // lanes per pixel
constexpr int EST_PPI = 256 / EST_LPP;         // pixels per workgroup iteration

template <int NC>
__device__ __forceinline__ void est_head_pixel(const float* __restrict__ f, int Cin, const float* __restrict__ s_w, int l,
                                               float (&v)[4]) {
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = 0.0f;
    for (int g = l; g < Cin / 4; g += EST_LPP) {
        const f32x4 a = *(const f32x4*)(f + 4 * g);
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
            for (int e = 0; e < 4; ++e) v[c] = fmaf(s_w[c * Cin + 4 * g + e], a[e], v[c]);
    }
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int o = EST_LPP / 2; o > 0; o >>= 1) v[c] += __shfl_xor(v[c], o);
}

template <int NC>
__global__ __launch_bounds__(256) void est_head_kernel(const float* __restrict__ feat, int Cin, long long HW,
                                                       const float* __restrict__ w, const float* __restrict__ bias, int sq,
                                                       float* __restrict__ map, double* __restrict__ partial) {
    extern __shared__ float s_w[];             // [NC][Cin]
    __shared__ double s_red[EST_PPI][4];
    const int tid = threadIdx.x, l = tid % EST_LPP, pg = tid / EST_LPP;
    const int n = blockIdx.y, nblk = gridDim.x;
    for (int i = tid; i < NC * Cin; i += 256) s_w[i] = w[i];
    __syncthreads();
    float b[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) b[c] = c < NC ? bias[c] : 0.0f;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    const float* fn = feat + (size_t)n * HW * Cin;
    for (long long p = ((long long)blockIdx.x * EST_PPI) + pg; p < HW; p += (long long)nblk * EST_PPI) {
        float v[4];
        est_head_pixel<NC>(fn + (size_t)p * Cin, Cin, s_w, l, v);
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            float y = v[c] + b[c];
            if (sq) y = y * y;
            if (partial) acc[c] += (double)y;
            else if (l == c) map[((size_t)n * NC + c) * HW + p] = y;
        }
    }
    if (!partial) return;
    if (l == 0)
#pragma unroll
        for (int c = 0; c < 4; ++c) s_red[pg][c] = acc[c];
    __syncthreads();
    if (tid < NC) {
        double s = 0.0;
        for (int j = 0; j < EST_PPI; ++j) s += s_red[j][tid];
        partial[((size_t)n * nblk + blockIdx.x) * NC + tid] = s;
    }
}

template <int NC>
__global__ __launch_bounds__(256) void est_head_finish_kernel(const double* __restrict__ partial, int nblk, long long HW,
                                                              float* __restrict__ mean) {
    __shared__ double s_red[256][4];
    const int tid = threadIdx.x, n = blockIdx.x;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int j = tid; j < nblk; j += 256)
#pragma unroll
        for (int c = 0; c < NC; ++c) acc[c] += partial[((size_t)n * nblk + j) * NC + c];
#pragma unroll
    for (int c = 0; c < 4; ++c) s_red[tid][c] = acc[c];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s)
#pragma unroll
            for (int c = 0; c < 4; ++c) s_red[tid][c] += s_red[tid + s][c];
        __syncthreads();
    }
    if (tid < NC) mean[n * NC + tid] = (float)(s_red[0][tid] / (double)HW);
}

extern "C" int yond_est_head_f32(const float* feat, int N, int H, int W, int Cin, const float* w, const float* bias, int out_nc,
                                 int sq, int pge, float* out, double* partial, void* stream) {
    if (!feat || !w || !bias || !out || N <= 0 || H <= 0 || W <= 0 || N > 65535) return YOND_EINVAL;
    if (out_nc < 1 || out_nc > 4 || Cin <= 0 || Cin % 4 != 0 || Cin > 4096) return YOND_EUNSUPPORTED;
    // the weights [out_nc][Cin] (dynamic LDS) sit beside s_red (static, EST_PPI x 4 doubles): together they must fit the 64 KiB a
    // workgroup gets without hipFuncSetAttribute, or the launch fails.  Cin = 4096 with out_nc = 4 is 64 KiB + 512 B: refused.
    if ((size_t)out_nc * Cin * sizeof(float) + EST_PPI * 4 * sizeof(double) > 65536) return YOND_EUNSUPPORTED;
    if (pge && !partial) return YOND_EINVAL;
    const long long HW = (long long)H * W;
    const long long groups = (HW + EST_PPI - 1) / EST_PPI;
    const int nblk = (int)(groups < YOND_EST_HEAD_BLOCKS ? groups : YOND_EST_HEAD_BLOCKS);
    const size_t lds = (size_t)out_nc * Cin * sizeof(float);
    hipStream_t st = (hipStream_t)stream;
    double* part = pge ? partial : nullptr;
    float* map = pge ? nullptr : out;
    switch (out_nc) {
        case 1: hipLaunchKernelGGL(est_head_kernel<1>, dim3(nblk, N), dim3(256), lds, st, feat, Cin, HW, w, bias, sq, map, part); break;
        case 2: hipLaunchKernelGGL(est_head_kernel<2>, dim3(nblk, N), dim3(256), lds, st, feat, Cin, HW, w, bias, sq, map, part); break;
        case 3: hipLaunchKernelGGL(est_head_kernel<3>, dim3(nblk, N), dim3(256), lds, st, feat, Cin, HW, w, bias, sq, map, part); break;
        default: hipLaunchKernelGGL(est_head_kernel<4>, dim3(nblk, N), dim3(256), lds, st, feat, Cin, HW, w, bias, sq, map, part); break;
    }
    YOND_LAUNCH_CHECK();
    if (!pge) return YOND_OK;
    switch (out_nc) {
        case 1: hipLaunchKernelGGL(est_head_finish_kernel<1>, dim3(N), dim3(256), 0, st, partial, nblk, HW, out); break;
        case 2: hipLaunchKernelGGL(est_head_finish_kernel<2>, dim3(N), dim3(256), 0, st, partial, nblk, HW, out); break;
        case 3: hipLaunchKernelGGL(est_head_finish_kernel<3>, dim3(N), dim3(256), 0, st, partial, nblk, HW, out); break;
        default: hipLaunchKernelGGL(est_head_finish_kernel<4>, dim3(N), dim3(256), 0, st, partial, nblk, HW, out); break;
    }
    YOND_LAUNCH_CHECK();
    return YOND_OK;
}

extern "C" size_t yond_est_head_ws_bytes(int N, int out_nc) {
    if (N <= 0 || out_nc < 1 || out_nc > 4) return 0;
    return (size_t)N * YOND_EST_HEAD_BLOCKS * out_nc * sizeof(double);
}
