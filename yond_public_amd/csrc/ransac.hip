// K7r: the robust noise-level fit, utils/isp_algos.py:345-362 with ransac=True -- sklearn's RANSACRegressor around a
//      LinearRegression, min_samples = int(sqrt(n)), 100 trials, residual_threshold = MAD of y -- which the reference leaves
//      unused because it is "巨慢" on one host thread (YOND_SIDD.py:85, 113).
//
//   ransac_count / ransac_offsets / ransac_scatter   the selected (x = mean, y = var) pairs in the order of NumPy's var[img_lap < th]
//            on the reference's [h][w][4] arrays (YOND_SIDD.py:77, 105), with polyfit's non-saturation rule (:348-350) applied:
//            per-workgroup counts, one scan, one scatter -- the same output for the same input, no atomic append.
//   ransac_absdev        d = |y - median(y)| in float32, the operand of the second median of sklearn's default threshold.
//   ransac_trial_fit     one workgroup per trial: gather the trial's m samples, centred float64 sums, the line through them
//            (LinearRegression(fit_intercept=True) on X = [x, 1]: the constant column centres to zero and gets coefficient 0).
//   ransac_score         all n points against every trial's line, TB trials per sweep of the workgroup's points (held in registers):
//            r = |y - (a x + b)| in float64, inlier iff r <= thr; per trial the count and {Sx, Sy, Sxx, Sxy, Syy, Srr} over the
//            inliers -- what sklearn's R^2 and the final refit need.  Wave shuffles, then the workgroup's waves through LDS in a fixed
//            order, then per-workgroup partials.
//   ransac_finish        one workgroup per trial adds the partials in a fixed order.
// No float64 atomics anywhere: two runs give the same bits.  sklearn's selection loop and the 2x2 refit of the winner run on the
// host on the [T][10] table (pipeline._ransac_select).
#include "nle_common.h"

#define RS_THREADS 256
#define RS_WAVES (RS_THREADS / 64)
#define RS_TILE YOND_RANSAC_TILE          // pixels per workgroup of the compaction
#define RS_PTS 8                          // points per thread of the scoring pass
#define RS_CHUNK YOND_RANSAC_CHUNK        // points per workgroup of the scoring pass
#define RS_TB 4                           // trials per sweep of the points
#define RS_NSUM 7                         // count, Sx, Sy, Sxx, Sxy, Syy, Srr
#define RS_MAXT YOND_RANSAC_MAXT

static_assert(RS_CHUNK == RS_THREADS * RS_PTS, "scoring chunk");
static_assert(RS_TILE % RS_THREADS == 0, "compaction tile");
static_assert(RS_MAXT % RS_TB == 0, "trial blocks");

// ---- compaction --------------------------------------------------------------------------------------------------------------
// A thread owns one pixel and walks its nch channels: element (pixel, c) lies at c * npix + pixel of the planar maps and at
// pixel * nch + c of the reference's order.  flags bit c: selected (lap < th); bit 4 + c: selected and 1e-4 < mean < 0.8.
// With the SIDD_256 re-tiling (YOND_SIDD.py:65, 92-93: np.concatenate(np.split(rggb, 32, axis=-2), axis=-1)) the reference's array is
// [h][tile_w][32 * 4]: slot g of its pixel order is (row, column inside the tile, tile), i.e. pixel row * 32 tile_w + tile * tile_w + j.
__device__ __forceinline__ size_t rs_pixel(size_t g, int tile_w) {
    if (tile_w == 0) return g;
    const size_t tile = g & 31, q = g >> 5;
    const size_t j = q % (size_t)tile_w, row = q / (size_t)tile_w;
    return row * 32 * (size_t)tile_w + tile * (size_t)tile_w + j;
}

__device__ __forceinline__ unsigned int rs_flags(const float* __restrict__ lap, const float* __restrict__ mean, size_t npix, int nch,
                                                 size_t pix, double th) {
    unsigned int f = 0;
    if (pix != (size_t)-1) {
        for (int c = 0; c < nch; ++c) {
            const size_t e = (size_t)c * npix + pix;
            const bool sel = lap ? ((double)lap[e] < th) : (0.0 < th);
            const float m = mean[e];
            const bool ns = sel && (m > 1e-4f) && (m < 0.8f);
            f |= (sel ? 1u : 0u) << c;
            f |= (ns ? 1u : 0u) << (4 + c);
        }
    }
    return f;
}

__device__ __forceinline__ unsigned int wave_incl_scan_u32(unsigned int v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned int up = __shfl_up(v, o);
        if (lane >= o) v += up;
    }
    return v;
}

// the non-saturation comparison of the reference runs on float32 x against the Python scalars 1e-4 and 0.8: NumPy compares in
// float32 with the scalars rounded to float32 (NEP 50), which is what (m > 1e-4f) && (m < 0.8f) does.
__global__ __launch_bounds__(RS_THREADS) void ransac_count_kernel(const float* __restrict__ lap, const float* __restrict__ mean, size_t npix,
                                                                  int nch, int tile_w, const double* __restrict__ th_p,
                                                                  unsigned int* __restrict__ counts) {
    __shared__ unsigned int s_c[RS_WAVES][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double th = *th_p;
    unsigned int call = 0, cns = 0;
    for (int j = 0; j < RS_TILE / RS_THREADS; ++j) {
        const size_t g = (size_t)blockIdx.x * RS_TILE + (size_t)j * RS_THREADS + tid;
        const size_t pix = g < npix ? rs_pixel(g, tile_w) : (size_t)-1;
        const unsigned int f = rs_flags(lap, mean, npix, nch, pix, th);
        call += __popc(f & 0xFu);
        cns += __popc(f >> 4);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        call += __shfl_xor(call, o);
        cns += __shfl_xor(cns, o);
    }
    if (lane == 0) { s_c[wave][0] = call; s_c[wave][1] = cns; }
    __syncthreads();
    if (tid < 2) {
        unsigned int s = 0;
        for (int w = 0; w < RS_WAVES; ++w) s += s_c[w][tid];
        counts[2 * (size_t)blockIdx.x + tid] = s;
    }
}

// one workgroup: totals, the 1 % rule (utils/isp_algos.py:349: len(x[nonsat]) > 0.01 * len(x)), exclusive offsets of the kept set
__global__ __launch_bounds__(1024) void ransac_offsets_kernel(const unsigned int* __restrict__ counts, unsigned int nwg,
                                                              unsigned long long* __restrict__ offs, long long* __restrict__ result) {
    __shared__ unsigned long long s_w[16][2];
    __shared__ int s_use;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned int per = (nwg + 1023u) / 1024u;
    const unsigned int w0 = (unsigned int)tid * per;
    unsigned long long a = 0, b = 0;
    for (unsigned int i = 0; i < per; ++i) {
        const unsigned int w = w0 + i;
        if (w < nwg) { a += counts[2 * (size_t)w]; b += counts[2 * (size_t)w + 1]; }
    }
    unsigned long long ia = wave_incl_scan_u64(a, lane), ib = wave_incl_scan_u64(b, lane);
    if (lane == 63) { s_w[wave][0] = ia; s_w[wave][1] = ib; }
    __syncthreads();
    unsigned long long ta = 0, tb = 0;
    for (int w = 0; w < 16; ++w) {
        if (w < wave) { ia += s_w[w][0]; ib += s_w[w][1]; }
        ta += s_w[w][0];
        tb += s_w[w][1];
    }
    if (tid == 0) {
        const int use = ((double)tb > 0.01 * (double)ta) ? 1 : 0;
        s_use = use;
        result[0] = (long long)(use ? tb : ta);              // n: the points handed to the fit
        result[1] = (long long)ta;                           // selected before the non-saturation rule
        result[2] = use;
    }
    __syncthreads();
    const int use = s_use;
    unsigned long long run = use ? (ib - b) : (ia - a);
    for (unsigned int i = 0; i < per; ++i) {
        const unsigned int w = w0 + i;
        if (w < nwg) {
            offs[w] = run;
            run += counts[2 * (size_t)w + use];
        }
    }
}

__global__ __launch_bounds__(RS_THREADS) void ransac_scatter_kernel(const float* __restrict__ lap, const float* __restrict__ mean,
                                                                    const float* __restrict__ var, size_t npix, int nch, int tile_w,
                                                                    const double* __restrict__ th_p, const unsigned long long* __restrict__ offs,
                                                                    const long long* __restrict__ result, float* __restrict__ x,
                                                                    float* __restrict__ y) {
    __shared__ unsigned int s_w[RS_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double th = *th_p;
    const int shift = result[2] ? 4 : 0;
    unsigned long long base = offs[blockIdx.x];
    for (int j = 0; j < RS_TILE / RS_THREADS; ++j) {
        const size_t g = (size_t)blockIdx.x * RS_TILE + (size_t)j * RS_THREADS + tid;
        const size_t pix = g < npix ? rs_pixel(g, tile_w) : (size_t)-1;
        const unsigned int f = (rs_flags(lap, mean, npix, nch, pix, th) >> shift) & 0xFu;
        const unsigned int c = __popc(f);
        const unsigned int incl = wave_incl_scan_u32(c, lane);
        __syncthreads();                                     // (s_w of the previous round has been read)
        if (lane == 63) s_w[wave] = incl;
        __syncthreads();
        unsigned int before = incl - c, total = 0;
        for (int w = 0; w < RS_WAVES; ++w) {
            if (w < wave) before += s_w[w];
            total += s_w[w];
        }
        unsigned long long o = base + before;
        for (int ch = 0; ch < nch; ++ch) {
            if ((f >> ch) & 1u) {
                const size_t e = (size_t)ch * npix + pix;
                x[o] = mean[e];
                y[o] = var[e];
                ++o;
            }
        }
        base += total;
    }
}

extern "C" size_t yond_ransac_compact_ws_bytes(size_t npix) {
    const size_t nwg = (npix + RS_TILE - 1) / RS_TILE;
    return nwg * (2 * sizeof(unsigned int) + sizeof(unsigned long long)) + 64;
}

extern "C" int yond_ransac_compact_f32(const float* lap, const float* mean, const float* var, size_t npix, int nch, int tile_w,
                                       const double* th, float* x, float* y, long long* result, void* ws, void* stream) {
    if (!mean || !var || !th || !x || !y || !result || !ws || npix == 0 || nch < 1 || nch > 4) return YOND_EINVAL;
    if (tile_w < 0 || (tile_w > 0 && npix % (32 * (size_t)tile_w))) return YOND_EINVAL;      // whole rows of 32 tiles
    if ((uintptr_t)ws & 7) return YOND_EINVAL;
    const size_t nwg = (npix + RS_TILE - 1) / RS_TILE;
    if (nwg > 0x7FFFFFFFull || npix > (size_t)0xFFFFFFFFull) return YOND_EUNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* offs = (unsigned long long*)ws;                       // [nwg]
    unsigned int* counts = (unsigned int*)(offs + nwg);                       // [nwg][2]
    hipLaunchKernelGGL(ransac_count_kernel, dim3((unsigned)nwg), dim3(RS_THREADS), 0, st, lap, mean, npix, nch, tile_w, th, counts);
    YOND_LAUNCH_CHECK();
    hipLaunchKernelGGL(ransac_offsets_kernel, dim3(1), dim3(1024), 0, st, (const unsigned int*)counts, (unsigned int)nwg, offs, result);
    YOND_LAUNCH_CHECK();
    hipLaunchKernelGGL(ransac_scatter_kernel, dim3((unsigned)nwg), dim3(RS_THREADS), 0, st, lap, mean, var, npix, nch, tile_w, th,
                       (const unsigned long long*)offs, (const long long*)result, x, y);
    YOND_LAUNCH_CHECK();
    return YOND_OK;
}

// ---- residual threshold ------------------------------------------------------------------------------------------------------
// np.median of a float32 array: the mean of the two middle order statistics in float32 ((a + b) / 2; a == b for odd n)
__device__ __forceinline__ float rs_median2(const float* __restrict__ v2) {
    return __fdiv_rn(__fadd_rn(v2[0], v2[1]), 2.0f);
}

__global__ __launch_bounds__(RS_THREADS) void ransac_absdev_kernel(const float* __restrict__ y, size_t n, const float* __restrict__ med2,
                                                                   float* __restrict__ d) {
    const float med = rs_median2(med2);
    for (size_t i = (size_t)blockIdx.x * RS_THREADS + threadIdx.x; i < n; i += (size_t)gridDim.x * RS_THREADS)
        d[i] = fabsf(__fsub_rn(y[i], med));
}

extern "C" int yond_ransac_absdev_f32(const float* y, size_t n, const float* med2, float* d, void* stream) {
    if (!y || !med2 || !d || n == 0) return YOND_EINVAL;
    size_t nb = (n + RS_THREADS - 1) / RS_THREADS;
    if (nb > 4096) nb = 4096;
    hipLaunchKernelGGL(ransac_absdev_kernel, dim3((unsigned)nb), dim3(RS_THREADS), 0, (hipStream_t)stream, y, n, med2, d);
    YOND_LAUNCH_CHECK();
    return YOND_OK;
}

// ---- trial fits --------------------------------------------------------------------------------------------------------------
// the workgroup's sum of v in a fixed order: lanes by xor shuffles, waves in index order (every thread gets the same bits)
__device__ __forceinline__ double rs_block_sum(double v, double* s_red /* [RS_WAVES] */) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    for (int w = 0; w < RS_WAVES; ++w) s += s_red[w];
    return s;
}

__global__ __launch_bounds__(RS_THREADS) void ransac_trial_fit_kernel(const float* __restrict__ x, const float* __restrict__ y, size_t n,
                                                                      const int* __restrict__ idx, int m, const float* __restrict__ thr2,
                                                                      double* __restrict__ out) {
    __shared__ double s_red[RS_WAVES];
    const int tid = threadIdx.x, t = blockIdx.x;
    const int* ix = idx + (size_t)t * m;
    double sx = 0.0, sy = 0.0;
    for (int i = tid; i < m; i += RS_THREADS) {
        size_t j = (size_t)(unsigned int)ix[i];
        if (j >= n) j = 0;                                   // (the host checks the table; never read outside the arrays)
        sx += (double)x[j];
        sy += (double)y[j];
    }
    sx = rs_block_sum(sx, s_red);
    sy = rs_block_sum(sy, s_red);
    const double xm = sx / (double)m, ym = sy / (double)m;
    double sxx = 0.0, sxy = 0.0;
    for (int i = tid; i < m; i += RS_THREADS) {
        size_t j = (size_t)(unsigned int)ix[i];
        if (j >= n) j = 0;
        const double dx = (double)x[j] - xm, dy = (double)y[j] - ym;
        sxx += dx * dx;
        sxy += dx * dy;
    }
    sxx = rs_block_sum(sxx, s_red);
    sxy = rs_block_sum(sxy, s_red);
    if (tid == 0) {
        const double a = sxx > 0.0 ? sxy / sxx : 0.0;        // a constant subset: the minimum-norm solution of lstsq, slope 0
        double* o = out + (size_t)t * YOND_RANSAC_COLS;
        o[0] = a;
        o[1] = ym - xm * a;
        o[9] = (double)rs_median2(thr2);
    }
}

// ---- scoring -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RS_THREADS) void ransac_score_kernel(const float* __restrict__ x, const float* __restrict__ y, size_t n, int T,
                                                                  const float* __restrict__ thr2, const double* __restrict__ lines,
                                                                  double* __restrict__ partial) {
    __shared__ double s_p[RS_WAVES][RS_MAXT][RS_NSUM];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double thr = (double)rs_median2(thr2);
    double px[RS_PTS], py[RS_PTS];
    const double qnan = __longlong_as_double(0x7FF8000000000000ll);
#pragma unroll
    for (int j = 0; j < RS_PTS; ++j) {
        const size_t i = (size_t)blockIdx.x * RS_CHUNK + (size_t)j * RS_THREADS + tid;
        const bool ok = i < n;
        px[j] = ok ? (double)x[i] : 0.0;
        py[j] = ok ? (double)y[i] : qnan;                    // a point past the end has a NaN residual: never an inlier
    }
    for (int t0 = 0; t0 < T; t0 += RS_TB) {
        double a[RS_TB], b[RS_TB];
        int cnt[RS_TB];
        double acc[RS_TB][RS_NSUM - 1];
#pragma unroll
        for (int u = 0; u < RS_TB; ++u) {
            const int t = (t0 + u < T) ? (t0 + u) : (T - 1);  // (the last block may be short: its extra columns are not stored)
            a[u] = lines[(size_t)t * YOND_RANSAC_COLS];
            b[u] = lines[(size_t)t * YOND_RANSAC_COLS + 1];
            cnt[u] = 0;
#pragma unroll
            for (int k = 0; k < RS_NSUM - 1; ++k) acc[u][k] = 0.0;
        }
#pragma unroll
        for (int j = 0; j < RS_PTS; ++j) {
#pragma unroll
            for (int u = 0; u < RS_TB; ++u) {
                const double pred = a[u] * px[j] + b[u];
                const double r = fabs(py[j] - pred);
                const bool in = r <= thr;
                const double xv = in ? px[j] : 0.0, yv = in ? py[j] : 0.0, rv = in ? r : 0.0;
                cnt[u] += in ? 1 : 0;
                acc[u][0] += xv;
                acc[u][1] += yv;
                acc[u][2] += xv * xv;
                acc[u][3] += xv * yv;
                acc[u][4] += yv * yv;
                acc[u][5] += rv * rv;
            }
        }
#pragma unroll
        for (int u = 0; u < RS_TB; ++u) {
            int c = cnt[u];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
            double v[RS_NSUM - 1];
#pragma unroll
            for (int k = 0; k < RS_NSUM - 1; ++k) v[k] = wave_sum(acc[u][k]);
            if (lane == 0 && t0 + u < T) {
                s_p[wave][t0 + u][0] = (double)c;
#pragma unroll
                for (int k = 0; k < RS_NSUM - 1; ++k) s_p[wave][t0 + u][1 + k] = v[k];
            }
        }
    }
    __syncthreads();
    for (int e = tid; e < T * RS_NSUM; e += RS_THREADS) {
        const int t = e / RS_NSUM, k = e % RS_NSUM;
        double s = 0.0;
        for (int w = 0; w < RS_WAVES; ++w) s += s_p[w][t][k];
        partial[((size_t)blockIdx.x * T + t) * RS_NSUM + k] = s;
    }
}

__global__ __launch_bounds__(RS_THREADS) void ransac_finish_kernel(const double* __restrict__ partial, unsigned int nwg, int T,
                                                                   double* __restrict__ out) {
    __shared__ double s_red[RS_WAVES];
    const int tid = threadIdx.x, t = blockIdx.x;
    for (int k = 0; k < RS_NSUM; ++k) {
        double s = 0.0;
        for (unsigned int w = tid; w < nwg; w += RS_THREADS) s += partial[((size_t)w * T + t) * RS_NSUM + k];
        s = rs_block_sum(s, s_red);
        if (tid == 0) out[(size_t)t * YOND_RANSAC_COLS + 2 + k] = s;
    }
}

extern "C" size_t yond_ransac_ws_bytes(size_t n, int T) {
    if (T < 1 || T > RS_MAXT) return 0;
    const size_t nwg = (n + RS_CHUNK - 1) / RS_CHUNK;
    return nwg * (size_t)T * RS_NSUM * sizeof(double) + 64;
}

extern "C" int yond_ransac_trials_f32(const float* x, const float* y, size_t n, const int32_t* idx, int T, int m, const float* thr2,
                                      double* out, void* ws, void* stream) {
    if (!x || !y || !idx || !thr2 || !out || !ws || n < 2 || T < 1 || T > RS_MAXT || m < 1 || (size_t)m > n) return YOND_EINVAL;
    if ((uintptr_t)ws & 7) return YOND_EINVAL;
    const size_t nwg = (n + RS_CHUNK - 1) / RS_CHUNK;
    if (nwg > 0x7FFFFFFFull || n > (size_t)0xFFFFFFFFull) return YOND_EUNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    double* partial = (double*)ws;
    hipLaunchKernelGGL(ransac_trial_fit_kernel, dim3((unsigned)T), dim3(RS_THREADS), 0, st, x, y, n, (const int*)idx, m, thr2, out);
    YOND_LAUNCH_CHECK();
    hipLaunchKernelGGL(ransac_score_kernel, dim3((unsigned)nwg), dim3(RS_THREADS), 0, st, x, y, n, T, thr2, (const double*)out, partial);
    YOND_LAUNCH_CHECK();
    hipLaunchKernelGGL(ransac_finish_kernel, dim3((unsigned)T), dim3(RS_THREADS), 0, st, (const double*)partial, (unsigned int)nwg, T, out);
    YOND_LAUNCH_CHECK();
    return YOND_OK;
}
