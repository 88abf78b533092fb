// Training-mode BatchNorm2d + ReLU and its backward for the DnCNN training step (archs/comp.py:18-26: Conv2d(no bias) ->
// BatchNorm2d(nf, eps 1e-4, momentum 0.95) -> ReLU), on [N][H][W][C] float32 tensors seen as [M = N H W pixels][C], C = 32, 64, 96, 128.
//   stats       per channel Sy = sum y, Syy = sum y y in float64 (y y of a float32 is exact there): every workgroup stores its partial sums,
//               a one-workgroup finish adds them in a fixed order and writes mean, rstd = 1 / sqrt(var_biased + eps), the epilogue pair
//               scale = gamma rstd, shift = beta - mean scale (formed in float64, rounded once each, as dncnn.fold_batchnorm does on the host)
//               and the PENDING running statistics (the caller commits them once the step's verdict is in)
//   apply       out = max(fmaf(y, scale, shift), 0)
//   bwd reduce  g = dout [fmaf(y, scale, shift) > 0], yh = (y - mean) rstd:  dbeta = sum g, dgamma = sum g yh  (float64 partials, fixed order)
//   bwd apply   dy = scale (g - dbeta / M - yh dgamma / M)
// The ReLU mask of the two backward kernels is RECOMPUTED with the forward's own fmaf on the same three float32 values (bn_act below is
// the one place that forms it), not stored: one more FMA per element instead of another tensor of traffic.
// All four stream HBM: a thread owns four channels (one 16-byte access per tensor and pixel), 256 / (C / 4) pixels per workgroup pass
// (C = 96: 10 pixels, 240 of the 256 threads), the per-channel constants sit in registers.  No float atomics anywhere: the results
// are bitwise reproducible from run to run (a captured step is compared with an eager one).
#include "common.h"

namespace {

constexpr int BN_MAX_WG = 1024;          // workgroups of a streaming launch = partial sums the finish adds per channel
constexpr int BN_PIX_PER_THREAD = 8;     // below BN_MAX_WG workgroups: about this many pixels per thread

struct BnGeom {
    int c4, ppw, nwg;
};

bool bn_shape_ok(size_t M, int C) { return M >= 2 && C >= 32 && C <= 128 && C % 32 == 0; }

BnGeom bn_geom(size_t M, int C) {
    BnGeom g;
    g.c4 = C / 4;
    g.ppw = 256 / g.c4;
    const size_t per = (size_t)g.ppw * BN_PIX_PER_THREAD;
    size_t n = (M + per - 1) / per;
    g.nwg = (int)(n < 1 ? 1 : n > (size_t)BN_MAX_WG ? (size_t)BN_MAX_WG : n);
    return g;
}

template <typename... P>
bool bn_aligned(unsigned long long mask, const P*... p) { return (((unsigned long long)p | ...) & mask) == 0; }

// the forward's pre-activation: the ONE expression every kernel forms it with (an explicit fused multiply-add, never contracted differently)
__device__ __forceinline__ float bn_act(float y, float scale, float shift) { return __builtin_fmaf(y, scale, shift); }

// Two float64 sums per channel and workgroup: LDS [256][8] doubles, then thread t < 2 C adds the ppw pixel rows of (sum t / C, channel t % C)
// in row order and stores ws[(wg * 2 + sum) * C + channel].
__device__ __forceinline__ void bn_store_partials(double (*s)[8], const double a[8], int C, int c4, int ppw, double* __restrict__ ws) {
    const int t = threadIdx.x;
#pragma unroll
    for (int e = 0; e < 8; ++e) s[t][e] = a[e];
    __syncthreads();
    if (t < 2 * C) {
        const int which = t / C, ch = t % C;
        const int grp = ch >> 2, e = (ch & 3) + 4 * which;
        double acc = 0.0;
        for (int r = 0; r < ppw; ++r) acc += s[r * c4 + grp][e];
        ws[((size_t)blockIdx.x * 2 + which) * C + ch] = acc;
    }
}

__global__ __launch_bounds__(256) void bn_stats_kernel(const float* __restrict__ y, long long M, int C, double* __restrict__ ws) {
    __shared__ double s[256][8];
    const int c4 = C / 4, ppw = 256 / c4;
    const int cl = threadIdx.x % c4, pr = threadIdx.x / c4;
    double a[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (pr < ppw) {
        const long long stride = (long long)gridDim.x * ppw;
        long long p = (long long)blockIdx.x * ppw + pr;
        for (; p + stride < M; p += 2 * stride) {             // two loads in flight
            const float4 u = *(const float4*)(y + p * C + cl * 4);
            const float4 v = *(const float4*)(y + (p + stride) * C + cl * 4);
            const double u0 = u.x, u1 = u.y, u2 = u.z, u3 = u.w, v0 = v.x, v1 = v.y, v2 = v.z, v3 = v.w;
            a[0] += u0; a[1] += u1; a[2] += u2; a[3] += u3;
            a[4] += u0 * u0; a[5] += u1 * u1; a[6] += u2 * u2; a[7] += u3 * u3;
            a[0] += v0; a[1] += v1; a[2] += v2; a[3] += v3;
            a[4] += v0 * v0; a[5] += v1 * v1; a[6] += v2 * v2; a[7] += v3 * v3;
        }
        if (p < M) {
            const float4 u = *(const float4*)(y + p * C + cl * 4);
            const double u0 = u.x, u1 = u.y, u2 = u.z, u3 = u.w;
            a[0] += u0; a[1] += u1; a[2] += u2; a[3] += u3;
            a[4] += u0 * u0; a[5] += u1 * u1; a[6] += u2 * u2; a[7] += u3 * u3;
        }
    }
    bn_store_partials(s, a, C, c4, ppw, ws);
}

// The finish of both reductions: one workgroup of 256 threads, thread = (slice, channel) with 256 / C slices (C = 96: 2, 192 threads);
// slice k adds the partials of workgroups k, k + slices, ... in that order, slice 0 then adds the slices' sums in slice order.
__device__ __forceinline__ void bn_finish_sums(const double* __restrict__ ws, int nwg, int C, double (*s)[256], double& s0, double& s1) {
    const int slices = 256 / C;
    const int ch = threadIdx.x % C, sl = threadIdx.x / C;
    double a0 = 0.0, a1 = 0.0;
    if (sl < slices)
        for (int g = sl; g < nwg; g += slices) {
            a0 += ws[((size_t)g * 2 + 0) * C + ch];
            a1 += ws[((size_t)g * 2 + 1) * C + ch];
        }
    s[0][threadIdx.x] = a0;
    s[1][threadIdx.x] = a1;
    __syncthreads();
    s0 = 0.0;
    s1 = 0.0;
    if (sl == 0)
        for (int k = 0; k < slices; ++k) {
            s0 += s[0][k * C + ch];
            s1 += s[1][k * C + ch];
        }
}

__global__ __launch_bounds__(256) void bn_stats_finish_kernel(const double* __restrict__ ws, int nwg, long long M, int C,
                                                              const float* __restrict__ gamma, const float* __restrict__ beta,
                                                              const float* __restrict__ rm, const float* __restrict__ rv, double eps,
                                                              double momentum, float* __restrict__ stat, float* __restrict__ pending) {
    __shared__ double s[2][256];
    double sy, syy;
    bn_finish_sums(ws, nwg, C, s, sy, syy);
    if (threadIdx.x < C) {
        const int ch = threadIdx.x;
        const double m = (double)M;
        const double mean = sy / m;
        double var = (syy - sy * mean) / m;                   // biased; a constant channel may land a rounding below zero
        var = var < 0.0 ? 0.0 : var;                          // (NaN stays NaN: the comparison is false)
        const double rstd = 1.0 / sqrt(var + eps);
        const double scale = (double)gamma[ch] * rstd;
        const double shift = (double)beta[ch] - mean * scale;
        stat[ch] = (float)mean;
        stat[C + ch] = (float)rstd;
        stat[2 * C + ch] = (float)scale;
        stat[3 * C + ch] = (float)shift;
        pending[ch] = (float)((1.0 - momentum) * (double)rm[ch] + momentum * mean);
        pending[C + ch] = (float)((1.0 - momentum) * (double)rv[ch] + momentum * (var * (m / (m - 1.0))));
    }
}

__global__ __launch_bounds__(256) void bn_bwd_finish_kernel(const double* __restrict__ ws, int nwg, int C, float* __restrict__ dgamma,
                                                            float* __restrict__ dbeta) {
    __shared__ double s[2][256];
    double sg, sgy;
    bn_finish_sums(ws, nwg, C, s, sg, sgy);
    if (threadIdx.x < C) {
        dbeta[threadIdx.x] = (float)sg;
        dgamma[threadIdx.x] = (float)sgy;
    }
}

__global__ __launch_bounds__(256) void bn_apply_relu_kernel(const float* __restrict__ y, const float* __restrict__ stat, long long M, int C,
                                                            float* __restrict__ out) {
    const int c4 = C / 4, ppw = 256 / c4;
    const int cl = threadIdx.x % c4, pr = threadIdx.x / c4;
    if (pr >= ppw) return;
    const float4 k = *(const float4*)(stat + 2 * C + cl * 4), b = *(const float4*)(stat + 3 * C + cl * 4);
    const long long stride = (long long)gridDim.x * ppw;
    for (long long p = (long long)blockIdx.x * ppw + pr; p < M; p += stride) {
        const float4 v = *(const float4*)(y + p * C + cl * 4);
        const float t0 = bn_act(v.x, k.x, b.x), t1 = bn_act(v.y, k.y, b.y), t2 = bn_act(v.z, k.z, b.z), t3 = bn_act(v.w, k.w, b.w);
        float4 o;                                             // max(t, 0) that keeps a NaN (torch's ReLU does; fmaxf would drop it)
        o.x = t0 > 0.0f ? t0 : (t0 <= 0.0f ? 0.0f : t0);
        o.y = t1 > 0.0f ? t1 : (t1 <= 0.0f ? 0.0f : t1);
        o.z = t2 > 0.0f ? t2 : (t2 <= 0.0f ? 0.0f : t2);
        o.w = t3 > 0.0f ? t3 : (t3 <= 0.0f ? 0.0f : t3);
        *(float4*)(out + p * C + cl * 4) = o;
    }
}

__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const float* __restrict__ y, const float* __restrict__ dout,
                                                            const float* __restrict__ stat, long long M, int C, double* __restrict__ ws) {
    __shared__ double s[256][8];
    const int c4 = C / 4, ppw = 256 / c4;
    const int cl = threadIdx.x % c4, pr = threadIdx.x / c4;
    double a[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (pr < ppw) {
        const float4 mn4 = *(const float4*)(stat + cl * 4), rs4 = *(const float4*)(stat + C + cl * 4);
        const float4 k4 = *(const float4*)(stat + 2 * C + cl * 4), b4 = *(const float4*)(stat + 3 * C + cl * 4);
        const float mn[4] = {mn4.x, mn4.y, mn4.z, mn4.w}, rs[4] = {rs4.x, rs4.y, rs4.z, rs4.w};
        const float kk[4] = {k4.x, k4.y, k4.z, k4.w}, bb[4] = {b4.x, b4.y, b4.z, b4.w};
        const long long stride = (long long)gridDim.x * ppw;
        for (long long p = (long long)blockIdx.x * ppw + pr; p < M; p += stride) {
            const float4 v = *(const float4*)(y + p * C + cl * 4), d = *(const float4*)(dout + p * C + cl * 4);
            const float vv[4] = {v.x, v.y, v.z, v.w}, dd[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float g = bn_act(vv[e], kk[e], bb[e]) > 0.0f ? dd[e] : 0.0f;
                const float yh = (vv[e] - mn[e]) * rs[e];
                a[e] += (double)g;
                a[4 + e] += (double)g * (double)yh;           // (exact product of two float32)
            }
        }
    }
    bn_store_partials(s, a, C, c4, ppw, ws);
}

__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float* __restrict__ y, const float* __restrict__ dout,
                                                           const float* __restrict__ stat, const float* __restrict__ dgamma,
                                                           const float* __restrict__ dbeta, long long M, int C, float* __restrict__ dy) {
    const int c4 = C / 4, ppw = 256 / c4;
    const int cl = threadIdx.x % c4, pr = threadIdx.x / c4;
    if (pr >= ppw) return;
    const float4 mn4 = *(const float4*)(stat + cl * 4), rs4 = *(const float4*)(stat + C + cl * 4);
    const float4 k4 = *(const float4*)(stat + 2 * C + cl * 4), b4 = *(const float4*)(stat + 3 * C + cl * 4);
    const float4 dg4 = *(const float4*)(dgamma + cl * 4), db4 = *(const float4*)(dbeta + cl * 4);
    const float mn[4] = {mn4.x, mn4.y, mn4.z, mn4.w}, rs[4] = {rs4.x, rs4.y, rs4.z, rs4.w};
    const float kk[4] = {k4.x, k4.y, k4.z, k4.w}, bb[4] = {b4.x, b4.y, b4.z, b4.w};
    const float dg[4] = {dg4.x, dg4.y, dg4.z, dg4.w}, db[4] = {db4.x, db4.y, db4.z, db4.w};
    float mg[4], mb[4];                                       // dgamma / M, dbeta / M: divided in float64, rounded once
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        mg[e] = (float)((double)dg[e] / (double)M);
        mb[e] = (float)((double)db[e] / (double)M);
    }
    const long long stride = (long long)gridDim.x * ppw;
    for (long long p = (long long)blockIdx.x * ppw + pr; p < M; p += stride) {
        const float4 v = *(const float4*)(y + p * C + cl * 4), d = *(const float4*)(dout + p * C + cl * 4);
        const float vv[4] = {v.x, v.y, v.z, v.w}, dd[4] = {d.x, d.y, d.z, d.w};
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float g = bn_act(vv[e], kk[e], bb[e]) > 0.0f ? dd[e] : 0.0f;
            const float yh = (vv[e] - mn[e]) * rs[e];
            const float t = __builtin_fmaf(-yh, mg[e], g - mb[e]);
            o[e] = kk[e] * t;
        }
        *(float4*)(dy + p * C + cl * 4) = make_float4(o[0], o[1], o[2], o[3]);
    }
}

}  // namespace

extern "C" size_t yond_bn_train_ws_bytes(size_t M, int C) {
    if (!bn_shape_ok(M, C)) return 0;
    return (size_t)bn_geom(M, C).nwg * 2 * (size_t)C * sizeof(double);
}

extern "C" int yond_bn_stats_f32(const float* y, size_t M, int C, const float* gamma, const float* beta, const float* running_mean,
                                 const float* running_var, double eps, double momentum, float* stat, float* pending, void* ws,
                                 size_t ws_bytes, void* stream) {
    if (!y || !gamma || !beta || !running_mean || !running_var || !stat || !pending || !ws || !bn_shape_ok(M, C)) return YOND_EINVAL;
    if (!bn_aligned(15ull, y, stat) || !bn_aligned(7ull, (const char*)ws) || ws_bytes < yond_bn_train_ws_bytes(M, C)) return YOND_EINVAL;
    if (!(eps >= 0.0) || !(momentum >= 0.0 && momentum <= 1.0)) return YOND_EINVAL;
    const BnGeom g = bn_geom(M, C);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(bn_stats_kernel, dim3((unsigned)g.nwg), dim3(256), 0, st, y, (long long)M, C, (double*)ws);
    YOND_LAUNCH_CHECK();
    hipLaunchKernelGGL(bn_stats_finish_kernel, dim3(1), dim3(256), 0, st, (const double*)ws, g.nwg, (long long)M, C, gamma, beta, running_mean,
                       running_var, eps, momentum, stat, pending);
    YOND_LAUNCH_CHECK();
    return YOND_OK;
}

extern "C" int yond_bn_apply_relu_f32(const float* y, const float* stat, size_t M, int C, float* out, void* stream) {
    if (!y || !stat || !out || !bn_shape_ok(M, C) || !bn_aligned(15ull, y, stat, out)) return YOND_EINVAL;
    const BnGeom g = bn_geom(M, C);
    hipLaunchKernelGGL(bn_apply_relu_kernel, dim3((unsigned)g.nwg), dim3(256), 0, (hipStream_t)stream, y, stat, (long long)M, C, out);
    YOND_LAUNCH_CHECK();
    return YOND_OK;
}

extern "C" int yond_bn_bwd_reduce_f32(const float* y, const float* dout, const float* stat, size_t M, int C, float* dgamma, float* dbeta,
                                      void* ws, size_t ws_bytes, void* stream) {
    if (!y || !dout || !stat || !dgamma || !dbeta || !ws || !bn_shape_ok(M, C)) return YOND_EINVAL;
    if (!bn_aligned(15ull, y, dout, stat) || !bn_aligned(7ull, (const char*)ws) || ws_bytes < yond_bn_train_ws_bytes(M, C)) return YOND_EINVAL;
    const BnGeom g = bn_geom(M, C);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(bn_bwd_reduce_kernel, dim3((unsigned)g.nwg), dim3(256), 0, st, y, dout, stat, (long long)M, C, (double*)ws);
    YOND_LAUNCH_CHECK();
    hipLaunchKernelGGL(bn_bwd_finish_kernel, dim3(1), dim3(256), 0, st, (const double*)ws, g.nwg, C, dgamma, dbeta);
    YOND_LAUNCH_CHECK();
    return YOND_OK;
}

extern "C" int yond_bn_bwd_apply_f32(const float* y, const float* dout, const float* stat, const float* dgamma, const float* dbeta, size_t M,
                                     int C, float* dy, void* stream) {
    if (!y || !dout || !stat || !dgamma || !dbeta || !dy || !bn_shape_ok(M, C)) return YOND_EINVAL;
    if (!bn_aligned(15ull, y, dout, stat, dgamma, dbeta, dy)) return YOND_EINVAL;
    const BnGeom g = bn_geom(M, C);
    hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3((unsigned)g.nwg), dim3(256), 0, (hipStream_t)stream, y, dout, stat, dgamma, dbeta, (long long)M, C,
                       dy);
    YOND_LAUNCH_CHECK();
    return YOND_OK;
}
