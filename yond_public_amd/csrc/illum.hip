// M2: the ELD protocol's illuminance correction (data_process/__init__.py:139-171 IlluminanceCorrect.correct): one least-squares gain
// per frame between the clamped prediction and the unsaturated targets, applied before PSNR / SSIM.  The contract is in
// include/yond_hip.h.  House rules: asynchronous on the caller's stream, no allocation or synchronisation in the launch functions, no
// LDS staging, no scratch, no device printf / assert, no float64 atomics.
//   sums    one pass over pred and source (8 B per element): p = clamp(pred, 0, 1); where source != 1.0f the products p * source and
//           p * p (exact in float64) and a count go to one of four groups.  A lane keeps the 12 float64 sums in registers, a wave adds
//           them by shuffles, a workgroup through LDS in wave order, and writes its 12 partials to the workspace.  A second launch of one
//           workgroup of 1024 lanes adds the partials: lane t takes the partials t, t + 1024, ... in ascending order, a wave adds by
//           shuffles, the waves' sums are added in wave order.  The grid depends on n alone (one workgroup per YOND_ILLUM_BLOCK_ELEMS
//           elements up to YOND_ILLUM_MAX_BLOCKS, above it the fewest workgroups that make equally many passes of the stride loop),
//           so the order of every addition is a function of (n, layout, alignment): the same call gives the same bits.
//   apply   out = (float)(num / den) * clamp(pred, 0, 1), the gain read from the sums on the device (4 B in, 4 B out per element).
// Both take 16-byte accesses (ILLUM_UNROLL of them in flight per lane and array) when the pointers are 16-byte aligned and, for the
// BAYER layout, width % 4 == 0 -- a vector then lies in one row and starts at an even column; otherwise one element per lane.
// NaN: the clamp and the clip are comparisons with selects, which keep a NaN as torch.clamp does (fmaxf / fminf would return the bound).
#include "common.h"

#define ILLUM_T 256
#define ILLUM_UNROLL (YOND_ILLUM_BLOCK_ELEMS / (4 * ILLUM_T))
#define ILLUM_Q 12                          /* 4 groups x {num, den, count} */

static_assert(ILLUM_UNROLL * 4 * ILLUM_T == YOND_ILLUM_BLOCK_ELEMS && ILLUM_UNROLL >= 1, "YOND_ILLUM_BLOCK_ELEMS: a multiple of 4 * 256");

__device__ __forceinline__ float illum_clamp01(float x) { return x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x); }

// the three terms of one element; an excluded element adds zeros (a NaN prediction under a saturated target is left out with it)
struct IllumTerm {
    double num, den, cnt;
};
__device__ __forceinline__ IllumTerm illum_term(float pred, float source) {
    const bool incl = source != 1.0f;                                       // (a NaN target is included, as in torch)
    const double p = (double)illum_clamp01(pred), s = (double)source;
    IllumTerm t;
    t.num = incl ? p * s : 0.0;
    t.den = incl ? p * p : 0.0;
    t.cnt = incl ? 1.0 : 0.0;
    return t;
}

// a[3 * g + {0, 1, 2}] += t for the group g, with selects: a dynamic register index would go through scratch
__device__ __forceinline__ void illum_add(double (&a)[ILLUM_Q], int g, const IllumTerm& t) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        a[3 * k] += g == k ? t.num : 0.0;
        a[3 * k + 1] += g == k ? t.den : 0.0;
        a[3 * k + 2] += g == k ? t.cnt : 0.0;
    }
}

// group of element i (scalar path); BAYER comes with n < 2^32: 32-bit division
template <int LAYOUT>
__device__ __forceinline__ int illum_group(size_t i, int width) {
    if constexpr (LAYOUT == YOND_ILLUM_BAYER) {
        const uint32_t y = (uint32_t)i / (uint32_t)width, x = (uint32_t)i - y * (uint32_t)width;
        return (int)((y & 1u) * 2u + (x & 1u));
    } else if constexpr (LAYOUT == YOND_ILLUM_PACKED4) {
        return (int)(i & 3u);
    } else {
        return 0;
    }
}

// wave shuffles, then the four waves through LDS in wave order: thread q < 12 returns the workgroup's sum of quantity q
__device__ __forceinline__ double illum_block_sum(double (&a)[ILLUM_Q], double (*s_red)[ILLUM_Q]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int q = 0; q < ILLUM_Q; ++q) a[q] = wave_sum(a[q]);
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < ILLUM_Q; ++q) s_red[wave][q] = a[q];
    }
    __syncthreads();
    return tid < ILLUM_Q ? (s_red[0][tid] + s_red[1][tid]) + (s_red[2][tid] + s_red[3][tid]) : 0.0;
}

template <int LAYOUT>
__global__ __launch_bounds__(ILLUM_T) void illum_sums_kernel(const float* __restrict__ pred, const float* __restrict__ source, size_t n,
                                                             int width, int vec_ok, double* __restrict__ partial) {
    __shared__ double s_red[4][ILLUM_Q];
    const int tid = threadIdx.x;
    double a[ILLUM_Q];
#pragma unroll
    for (int q = 0; q < ILLUM_Q; ++q) a[q] = 0.0;
    const size_t nvec = vec_ok ? n / 4 : 0;
    const size_t stride = (size_t)gridDim.x * ILLUM_T;
    for (size_t v = (size_t)blockIdx.x * ILLUM_T + tid; v < nvec; v += stride * ILLUM_UNROLL) {
        f32x4 P[ILLUM_UNROLL], S[ILLUM_UNROLL];
#pragma unroll
        for (int u = 0; u < ILLUM_UNROLL; ++u) {                            // every load issued before the first use
            const size_t vu = v + u * stride;
            const size_t idx = (vu < nvec ? vu : v) * 4;
            P[u] = *(const f32x4*)(pred + idx);
            S[u] = *(const f32x4*)(source + idx);
        }
#pragma unroll
        for (int u = 0; u < ILLUM_UNROLL; ++u) {
            const size_t vu = v + u * stride;
            if (vu < nvec) {
                const IllumTerm t0 = illum_term(P[u][0], S[u][0]), t1 = illum_term(P[u][1], S[u][1]);
                const IllumTerm t2 = illum_term(P[u][2], S[u][2]), t3 = illum_term(P[u][3], S[u][3]);
                if constexpr (LAYOUT == YOND_ILLUM_BAYER) {
                    // the vector starts at an even column of one row: elements 0, 2 are the row's first group, 1, 3 its second
                    const int g0 = (int)((((uint32_t)(vu * 4) / (uint32_t)width) & 1u) * 2u);
                    const IllumTerm e = {t0.num + t2.num, t0.den + t2.den, t0.cnt + t2.cnt};
                    const IllumTerm o = {t1.num + t3.num, t1.den + t3.den, t1.cnt + t3.cnt};
                    a[0] += g0 == 0 ? e.num : 0.0; a[1] += g0 == 0 ? e.den : 0.0; a[2] += g0 == 0 ? e.cnt : 0.0;
                    a[3] += g0 == 0 ? o.num : 0.0; a[4] += g0 == 0 ? o.den : 0.0; a[5] += g0 == 0 ? o.cnt : 0.0;
                    a[6] += g0 == 2 ? e.num : 0.0; a[7] += g0 == 2 ? e.den : 0.0; a[8] += g0 == 2 ? e.cnt : 0.0;
                    a[9] += g0 == 2 ? o.num : 0.0; a[10] += g0 == 2 ? o.den : 0.0; a[11] += g0 == 2 ? o.cnt : 0.0;
                } else if constexpr (LAYOUT == YOND_ILLUM_PACKED4) {
                    a[0] += t0.num; a[1] += t0.den; a[2] += t0.cnt;
                    a[3] += t1.num; a[4] += t1.den; a[5] += t1.cnt;
                    a[6] += t2.num; a[7] += t2.den; a[8] += t2.cnt;
                    a[9] += t3.num; a[10] += t3.den; a[11] += t3.cnt;
                } else {
                    a[0] += (t0.num + t1.num) + (t2.num + t3.num);
                    a[1] += (t0.den + t1.den) + (t2.den + t3.den);
                    a[2] += (t0.cnt + t1.cnt) + (t2.cnt + t3.cnt);
                }
            }
        }
    }
    // what the vectors leave: everything on the scalar path, up to 3 tail elements (FLAT) on the vector path
    for (size_t i = nvec * 4 + (size_t)blockIdx.x * ILLUM_T + tid; i < n; i += stride)
        illum_add(a, illum_group<LAYOUT>(i, width), illum_term(pred[i], source[i]));
    const double t = illum_block_sum(a, s_red);
    if (tid < ILLUM_Q) partial[(size_t)blockIdx.x * ILLUM_Q + tid] = t;
}

// one workgroup of ILLUM_FIN_T lanes: sums[g] = {num, den, count} of the four groups, sums[4] = (g0 + g1) + (g2 + g3).  Lane t adds the
// partials of the workgroups t, t + ILLUM_FIN_T, ... in ascending order (at most YOND_ILLUM_MAX_BLOCKS / ILLUM_FIN_T of them: every load is
// in flight at once), a wave adds by shuffles, and lane q < 12 adds the waves' sums of quantity q in wave order.
#define ILLUM_FIN_T 1024
#define ILLUM_FIN_PER ((YOND_ILLUM_MAX_BLOCKS + ILLUM_FIN_T - 1) / ILLUM_FIN_T)
__global__ __launch_bounds__(ILLUM_FIN_T) void illum_finish_kernel(const double* __restrict__ partial, unsigned nblocks, double* __restrict__ sums) {
    __shared__ double s_red[ILLUM_FIN_T / 64][ILLUM_Q];
    __shared__ double s_g[ILLUM_Q];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double v[ILLUM_FIN_PER][ILLUM_Q];
#pragma unroll
    for (int k = 0; k < ILLUM_FIN_PER; ++k) {
        const unsigned b = (unsigned)tid + (unsigned)k * ILLUM_FIN_T;
#pragma unroll
        for (int q = 0; q < ILLUM_Q; ++q) v[k][q] = b < nblocks ? partial[(size_t)b * ILLUM_Q + q] : 0.0;
    }
    double a[ILLUM_Q];
#pragma unroll
    for (int q = 0; q < ILLUM_Q; ++q) {
        a[q] = v[0][q];
#pragma unroll
        for (int k = 1; k < ILLUM_FIN_PER; ++k) a[q] += v[k][q];
        a[q] = wave_sum(a[q]);
    }
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < ILLUM_Q; ++q) s_red[wave][q] = a[q];
    }
    __syncthreads();
    if (tid < ILLUM_Q) {
        double t = s_red[0][tid];
#pragma unroll
        for (int w = 1; w < ILLUM_FIN_T / 64; ++w) t += s_red[w][tid];
        s_g[tid] = t;
        sums[tid] = t;
    }
    __syncthreads();
    if (tid < 3) sums[ILLUM_Q + tid] = (s_g[tid] + s_g[3 + tid]) + (s_g[6 + tid] + s_g[9 + tid]);
}

// the four gains of an element's possible groups (FRAME: the total's, four times)
struct IllumGains {
    float g[4];
};
__device__ __forceinline__ IllumGains illum_gains(const double* __restrict__ sums, int mode) {
    IllumGains r;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int row = mode == YOND_ILLUM_CFA ? k : 4;
        r.g[k] = (float)(sums[3 * row] / sums[3 * row + 1]);               // IEEE: 0 / 0 and x / 0 as they come
    }
    return r;
}
__device__ __forceinline__ float illum_apply_one(float x, float gain, int clip) {
    float o = gain * illum_clamp01(x);
    if (clip) o = o > 1.0f ? 1.0f : o;
    return o;
}
__device__ __forceinline__ float illum_pick(const IllumGains& G, int g) {
    return g == 0 ? G.g[0] : (g == 1 ? G.g[1] : (g == 2 ? G.g[2] : G.g[3]));
}

// pred and out carry no __restrict__: they may be the same pointer (a lane reads the elements it writes before it writes them)
template <int LAYOUT>
__global__ __launch_bounds__(ILLUM_T) void illum_apply_kernel(const float* pred, size_t n, int width, int vec_ok, const double* __restrict__ sums,
                                                              int mode, int clip, float* out) {
    const int tid = threadIdx.x;
    const IllumGains G = illum_gains(sums, mode);
    const size_t nvec = vec_ok ? n / 4 : 0;
    const size_t stride = (size_t)gridDim.x * ILLUM_T;
    for (size_t v = (size_t)blockIdx.x * ILLUM_T + tid; v < nvec; v += stride * ILLUM_UNROLL) {
        f32x4 P[ILLUM_UNROLL];
#pragma unroll
        for (int u = 0; u < ILLUM_UNROLL; ++u) {
            const size_t vu = v + u * stride;
            P[u] = *(const f32x4*)(pred + (vu < nvec ? vu : v) * 4);
        }
#pragma unroll
        for (int u = 0; u < ILLUM_UNROLL; ++u) {
            const size_t vu = v + u * stride;
            if (vu < nvec) {
                float ge = G.g[0], go = G.g[0];                             // gains of the even and the odd elements (FLAT: group 0)
                float g2 = G.g[0], g3 = G.g[0];
                if constexpr (LAYOUT == YOND_ILLUM_BAYER) {
                    const bool odd_row = (((uint32_t)(vu * 4) / (uint32_t)width) & 1u) != 0;
                    ge = odd_row ? G.g[2] : G.g[0];
                    go = odd_row ? G.g[3] : G.g[1];
                    g2 = ge;
                    g3 = go;
                } else if constexpr (LAYOUT == YOND_ILLUM_PACKED4) {
                    go = G.g[1];
                    g2 = G.g[2];
                    g3 = G.g[3];
                }
                f32x4 o;
                o[0] = illum_apply_one(P[u][0], ge, clip);
                o[1] = illum_apply_one(P[u][1], go, clip);
                o[2] = illum_apply_one(P[u][2], g2, clip);
                o[3] = illum_apply_one(P[u][3], g3, clip);
                *(f32x4*)(out + vu * 4) = o;
            }
        }
    }
    for (size_t i = nvec * 4 + (size_t)blockIdx.x * ILLUM_T + tid; i < n; i += stride)
        out[i] = illum_apply_one(pred[i], illum_pick(G, illum_group<LAYOUT>(i, width)), clip);
}

// a function of n alone: one workgroup per YOND_ILLUM_BLOCK_ELEMS elements up to the cap; above it every workgroup makes the same number
// of passes of its stride loop (the last one partly): 2930 passes are 1465 workgroups of 2, not 2048 of which 882 go round twice
static unsigned illum_blocks(size_t n) {
    const size_t passes = ((n + 3) / 4 + (size_t)ILLUM_T * ILLUM_UNROLL - 1) / ((size_t)ILLUM_T * ILLUM_UNROLL);
    size_t cap = (size_t)yond_exp_long("YOND_ILLUM_WGS", YOND_ILLUM_MAX_BLOCKS);
    if (cap < 1 || cap > YOND_ILLUM_MAX_BLOCKS) cap = YOND_ILLUM_MAX_BLOCKS;      // (the workspace holds YOND_ILLUM_MAX_BLOCKS partials)
    if (passes <= cap) return (unsigned)(passes < 1 ? 1 : passes);
    const size_t rounds = (passes + cap - 1) / cap;
    return (unsigned)((passes + rounds - 1) / rounds);
}

// the geometry rules of a layout; YOND_OK or YOND_EINVAL
static int illum_geometry(size_t n, int width, int layout) {
    if (n == 0) return YOND_EINVAL;
    if (layout == YOND_ILLUM_BAYER) {
        if (width < 2 || (width & 1) || n > 0xffffffffull || n % (size_t)width || ((n / (size_t)width) & 1)) return YOND_EINVAL;
    } else if (layout == YOND_ILLUM_PACKED4) {
        if (n & 3) return YOND_EINVAL;
    } else if (layout != YOND_ILLUM_FLAT) {
        return YOND_EINVAL;
    }
    return YOND_OK;
}

extern "C" size_t yond_illum_ws_bytes(void) { return sizeof(double) * ILLUM_Q * YOND_ILLUM_MAX_BLOCKS; }

extern "C" int yond_illum_sums_f32(const float* pred, const float* source, size_t n, int width, int layout, double* sums, void* ws,
                                   void* stream) {
    if (!pred || !source || !sums || !ws) return YOND_EINVAL;
    if ((((uintptr_t)pred) | ((uintptr_t)source)) & 3u) return YOND_EINVAL;
    if ((((uintptr_t)sums) | ((uintptr_t)ws)) & 7u) return YOND_EINVAL;
    if (illum_geometry(n, width, layout) != YOND_OK) return YOND_EINVAL;
    const int vec_ok = !((((uintptr_t)pred) | ((uintptr_t)source)) & 15u) && (layout != YOND_ILLUM_BAYER || width % 4 == 0);
    const unsigned nb = illum_blocks(n);
    hipStream_t st = (hipStream_t)stream;
    double* partial = (double*)ws;
    if (layout == YOND_ILLUM_BAYER)
        hipLaunchKernelGGL(illum_sums_kernel<YOND_ILLUM_BAYER>, dim3(nb), dim3(ILLUM_T), 0, st, pred, source, n, width, vec_ok, partial);
    else if (layout == YOND_ILLUM_PACKED4)
        hipLaunchKernelGGL(illum_sums_kernel<YOND_ILLUM_PACKED4>, dim3(nb), dim3(ILLUM_T), 0, st, pred, source, n, width, vec_ok, partial);
    else
        hipLaunchKernelGGL(illum_sums_kernel<YOND_ILLUM_FLAT>, dim3(nb), dim3(ILLUM_T), 0, st, pred, source, n, width, vec_ok, partial);
    YOND_LAUNCH_CHECK();
    hipLaunchKernelGGL(illum_finish_kernel, dim3(1), dim3(ILLUM_FIN_T), 0, st, (const double*)partial, nb, sums);
    YOND_LAUNCH_CHECK();
    return YOND_OK;
}

extern "C" int yond_illum_apply_f32(const float* pred, size_t n, int width, int layout, const double* sums, int mode, int clip, float* out,
                                    void* stream) {
    if (!pred || !sums || !out) return YOND_EINVAL;
    if ((((uintptr_t)pred) | ((uintptr_t)out)) & 3u) return YOND_EINVAL;
    if (((uintptr_t)sums) & 7u) return YOND_EINVAL;
    if (mode != YOND_ILLUM_FRAME && mode != YOND_ILLUM_CFA) return YOND_EINVAL;
    if (illum_geometry(n, width, layout) != YOND_OK) return YOND_EINVAL;
    const int vec_ok = !((((uintptr_t)pred) | ((uintptr_t)out)) & 15u) && (layout != YOND_ILLUM_BAYER || width % 4 == 0);
    const unsigned nb = illum_blocks(n);
    hipStream_t st = (hipStream_t)stream;
    if (layout == YOND_ILLUM_BAYER)
        hipLaunchKernelGGL(illum_apply_kernel<YOND_ILLUM_BAYER>, dim3(nb), dim3(ILLUM_T), 0, st, pred, n, width, vec_ok, sums, mode, clip, out);
    else if (layout == YOND_ILLUM_PACKED4)
        hipLaunchKernelGGL(illum_apply_kernel<YOND_ILLUM_PACKED4>, dim3(nb), dim3(ILLUM_T), 0, st, pred, n, width, vec_ok, sums, mode, clip, out);
    else
        hipLaunchKernelGGL(illum_apply_kernel<YOND_ILLUM_FLAT>, dim3(nb), dim3(ILLUM_T), 0, st, pred, n, width, vec_ok, sums, mode, clip, out);
    YOND_LAUNCH_CHECK();
    return YOND_OK;
}
