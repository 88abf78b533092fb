// M5: row noise (banding) on a Bayer mosaic -- the reference's row_denoise, utils/isp_algos.py:319-334.  The contract is in
// include/yond_hip.h.  House rules: asynchronous on the caller's stream, no allocation or synchronisation in the launch functions, no
// scratch, no device printf / assert, no atomics.
//   sums    one wave takes one row at a time: a lane adds the elements it loads into two float64 accumulators (the two column phases; a
//           float4 holds both: x + z and y + w), the 64 lanes' pairs are combined by an xor-shuffle tree, lane 0 stores the row's pair.
//           The order of the additions is a function of W and of the path (16-byte loads / one element per lane) alone.
//   apply   the same wave-per-row walk.  A wave first computes its row's offsets from `sums`: lane t < d holds tap k = t - d / 2 (d <= 63),
//           its neighbour's mean, both weights and the product; numerator and denominator by the same shuffle tree.  Then it streams the
//           row: every element is read and written by one lane, so out may be in (exactly; a partial overlap is refused).
// Rows per pass are capped at RN_ROWS_CAP; a taller frame is walked in ceil(H / RN_ROWS_CAP) passes of equal size (a grid-stride loop),
// so that no wave has one row more than its share.
#include "common.h"
#include <math.h>

#define RN_T 256
#define RN_WAVES (RN_T / 64)
#define RN_DEPTH 4                          /* 16-byte loads a lane keeps in flight */
#define RN_ROWS_CAP 2048                    /* rows in flight: 512 workgroups of four waves */

static_assert(YOND_ROWNOISE_MAX_D < 64, "one tap per lane of a wave");

// the sum over the wave's 64 lanes, the same value (and the same order of additions) in every lane
__device__ __forceinline__ double rn_wave_sum(double v) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s);
    return v;
}

// the two float64 column-phase sums of one row, in every lane
template <bool VEC>
__device__ __forceinline__ void rn_row_sums(const float* __restrict__ row, int W, int lane, double& s0, double& s1) {
    double a0 = 0.0, a1 = 0.0;
    if constexpr (VEC) {
        const f32x4* row4 = (const f32x4*)row;
        const int n4 = W >> 2;
        for (int i = lane; i < n4; i += 64 * RN_DEPTH) {     // RN_DEPTH loads in flight (those past the row's end are skipped), added in
            f32x4 u[RN_DEPTH];                               // the order of the plain loop
#pragma unroll
            for (int e = 0; e < RN_DEPTH; ++e)
                if (i + 64 * e < n4) u[e] = row4[i + 64 * e];
#pragma unroll
            for (int e = 0; e < RN_DEPTH; ++e)
                if (i + 64 * e < n4) {
                    a0 += (double)u[e][0] + (double)u[e][2];
                    a1 += (double)u[e][1] + (double)u[e][3];
                }
        }
    } else {
        double a = 0.0;                                      // x = lane, lane + 64, ...: a lane stays on its column phase
        for (int x = lane; x < W; x += 64) a += (double)row[x];
        a0 = (lane & 1) ? 0.0 : a;
        a1 = (lane & 1) ? a : 0.0;
    }
    s0 = rn_wave_sum(a0);
    s1 = rn_wave_sum(a1);
}

template <bool VEC>
__global__ __launch_bounds__(RN_T) void rn_sums_kernel(const float* __restrict__ in, int H, int W, double* __restrict__ sums) {
    const int lane = threadIdx.x & 63;
    const int stride = gridDim.x * RN_WAVES;
    for (int y = blockIdx.x * RN_WAVES + (threadIdx.x >> 6); y < H; y += stride) {
        double s0, s1;
        rn_row_sums<VEC>(in + (size_t)y * W, W, lane, s0, s1);
        if (lane == 0) {
            sums[2 * (size_t)y] = s0;
            sums[2 * (size_t)y + 1] = s1;
        }
    }
}

__device__ __forceinline__ bool rn_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }    // false for NaN and the infinities

// the mean of row y's sequence: c < 0 the whole sensor row, else column phase c
__device__ __forceinline__ double rn_mean(const double* __restrict__ sums, int y, int c, double w_row, double w_plane) {
    const double s0 = sums[2 * (size_t)y], s1 = sums[2 * (size_t)y + 1];
    return c < 0 ? (s0 + s1) / w_row : (c ? s1 : s0) / w_plane;
}

// offset of row y (parity p, index j of n) for the sequence c: every lane returns the same value
__device__ __forceinline__ double rn_offset(const double* __restrict__ sums, int y, int n, int c, int d, int lane, double w_row, double w_plane,
                                            double ws, double two_sc2) {
    const int p = y & 1, j = y >> 1, r = d >> 1;
    const bool tap = lane < d;
    const int jk = min(max(j + lane - r, 0), n - 1);         // (a lane beyond the window reads a row of the frame and is not counted)
    const double mk = rn_mean(sums, 2 * jk + p, c, w_row, w_plane);
    const double m = __shfl(mk, r);                          // tap 0 is the row itself: j + 0 is never clamped
    const double dlt = m - mk;
    const double w = ws * exp(-(dlt * dlt) / two_sc2);
    const bool counted = tap && rn_finite(mk);
    double prod = w * dlt;
    const double num = rn_wave_sum(counted ? prod : 0.0);
    const double den = rn_wave_sum(counted ? w : 0.0);
    return rn_finite(m) ? num / den : 0.0;                   // (m finite: tap 0 has weight 1, den >= 1)
}

__device__ __forceinline__ float rn_sub(float v, double off, bool keep) { return keep ? v : (float)((double)v - off); }

template <bool VEC>
__global__ __launch_bounds__(RN_T) void rn_apply_kernel(const float* in, float* out, int H, int W, const double* __restrict__ sums, int per, int d,
                                                        double two_sc2, double two_ss2, double* __restrict__ offsets) {
    const int lane = threadIdx.x & 63;
    const int stride = gridDim.x * RN_WAVES;
    const int k = lane - (d >> 1);
    const double ws = exp(-(double)(k * k) / two_ss2);       // the lane's spatial weight: the same for every row
    const double w_row = (double)W, w_plane = (double)(W >> 1);
    for (int y = blockIdx.x * RN_WAVES + (threadIdx.x >> 6); y < H; y += stride) {
        double off0, off1;
        if (per == YOND_ROWNOISE_ROW) {
            off0 = off1 = rn_offset(sums, y, H >> 1, -1, d, lane, w_row, w_plane, ws, two_sc2);
        } else {
            off0 = rn_offset(sums, y, H >> 1, 0, d, lane, w_row, w_plane, ws, two_sc2);
            off1 = rn_offset(sums, y, H >> 1, 1, d, lane, w_row, w_plane, ws, two_sc2);
        }
        if (offsets && lane == 0) {
            offsets[2 * (size_t)y] = off0;
            offsets[2 * (size_t)y + 1] = off1;
        }
        const bool k0 = off0 == 0.0, k1 = off1 == 0.0;       // offset 0: the pixel passes through, bit for bit
        const float* src = in + (size_t)y * W;
        float* dst = out + (size_t)y * W;
        if constexpr (VEC) {
            const f32x4* src4 = (const f32x4*)src;
            f32x4* dst4 = (f32x4*)dst;
            const int n4 = W >> 2;
            for (int i = lane; i < n4; i += 64 * RN_DEPTH) {
                f32x4 u[RN_DEPTH];
#pragma unroll
                for (int e = 0; e < RN_DEPTH; ++e)
                    if (i + 64 * e < n4) u[e] = src4[i + 64 * e];
#pragma unroll
                for (int e = 0; e < RN_DEPTH; ++e)
                    if (i + 64 * e < n4)
                        dst4[i + 64 * e] = f32x4{rn_sub(u[e][0], off0, k0), rn_sub(u[e][1], off1, k1), rn_sub(u[e][2], off0, k0), rn_sub(u[e][3], off1, k1)};
            }
        } else {
            const double off = (lane & 1) ? off1 : off0;
            const bool keep = (lane & 1) ? k1 : k0;
            for (int x = lane; x < W; x += 64) dst[x] = rn_sub(src[x], off, keep);
        }
    }
}

// H and W even and >= 2, H * W < 2^31
static int rn_geometry(int H, int W) {
    if (H < 2 || W < 2 || (H & 1) || (W & 1)) return YOND_EINVAL;
    if ((unsigned long long)H * (unsigned long long)W >= (1ull << 31)) return YOND_EINVAL;
    return YOND_OK;
}

// workgroups of RN_WAVES rows: ceil(H / RN_ROWS_CAP) passes of equal size
static unsigned rn_grid(int H) {
    const int passes = (H + RN_ROWS_CAP - 1) / RN_ROWS_CAP;
    const int rows = (H + passes - 1) / passes;
    return (unsigned)((rows + RN_WAVES - 1) / RN_WAVES);
}

extern "C" int yond_rownoise_sums_f32(const float* in, int H, int W, double* sums, void* stream) {
    if (!in || !sums) return YOND_EINVAL;
    if ((((uintptr_t)in) & 3u) || (((uintptr_t)sums) & 7u)) return YOND_EINVAL;
    if (rn_geometry(H, W) != YOND_OK) return YOND_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (!(((uintptr_t)in) & 15u) && W % 4 == 0)
        hipLaunchKernelGGL(rn_sums_kernel<true>, dim3(rn_grid(H)), dim3(RN_T), 0, st, in, H, W, sums);
    else
        hipLaunchKernelGGL(rn_sums_kernel<false>, dim3(rn_grid(H)), dim3(RN_T), 0, st, in, H, W, sums);
    YOND_LAUNCH_CHECK();
    return YOND_OK;
}

extern "C" int yond_rownoise_apply_f32(const float* in, float* out, int H, int W, const double* sums, int per, int d, double sigma_color,
                                       double sigma_space, double* offsets, void* stream) {
    if (!in || !out || !sums) return YOND_EINVAL;
    if ((((uintptr_t)in) | ((uintptr_t)out)) & 3u) return YOND_EINVAL;
    if ((((uintptr_t)sums) | ((uintptr_t)offsets)) & 7u) return YOND_EINVAL;
    if (rn_geometry(H, W) != YOND_OK) return YOND_EINVAL;
    if (out != in) {                                         // in place, or apart: a frame shifted by some rows would race between waves
        const uintptr_t a = (uintptr_t)in, b = (uintptr_t)out, bytes = (uintptr_t)H * (uintptr_t)W * sizeof(float);
        if (a < b + bytes && b < a + bytes) return YOND_EINVAL;
    }
    if (d < 1 || d > YOND_ROWNOISE_MAX_D || !(d & 1)) return YOND_EINVAL;
    if (!(sigma_color > 0.0) || !(sigma_space > 0.0) || !isfinite(sigma_color) || !isfinite(sigma_space)) return YOND_EINVAL;
    if (per != YOND_ROWNOISE_ROW && per != YOND_ROWNOISE_PLANE) return YOND_EINVAL;
    const double two_sc2 = 2.0 * sigma_color * sigma_color, two_ss2 = 2.0 * sigma_space * sigma_space;
    if (!(two_sc2 > 0.0) || !(two_ss2 > 0.0)) return YOND_EINVAL;    // (a sigma whose square underflows: tap 0 would be exp(-0 / 0))
    hipStream_t st = (hipStream_t)stream;
    if (!((((uintptr_t)in) | ((uintptr_t)out)) & 15u) && W % 4 == 0)
        hipLaunchKernelGGL(rn_apply_kernel<true>, dim3(rn_grid(H)), dim3(RN_T), 0, st, in, out, H, W, sums, per, d, two_sc2, two_ss2, offsets);
    else
        hipLaunchKernelGGL(rn_apply_kernel<false>, dim3(rn_grid(H)), dim3(RN_T), 0, st, in, out, H, W, sums, per, d, two_sc2, two_ss2, offsets);
    YOND_LAUNCH_CHECK();
    return YOND_OK;
}
