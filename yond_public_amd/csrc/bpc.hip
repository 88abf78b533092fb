// M4: defective-pixel repair on a Bayer mosaic (utils/isp_ops.py:152-160 repair_bad_pixels, and this project's blind detection).  The
// contract is in include/yond_hip.h.  House rules: asynchronous on the caller's stream, no allocation or synchronisation in the launch
// functions, no scratch, no device printf / assert.
//   list     one lane per listed point: nine clamped reads of `in`, the median from the three sorted columns, one write to `out`.
//   detect   one pass over the frame.  A workgroup of 256 lanes takes a tile of YOND_BPC_TILE_H x YOND_BPC_TILE_W pixels: it stages the
//            tile with its two-pixel halo in LDS -- the CLAMPED same-colour coordinate is resolved while staging, so that the LDS cell of
//            (y, x) holds in[cy(y)][cx(x)] and the compute phase knows no border -- then every lane takes four pixels of a row in each
//            of four rows: three 32-byte LDS rows give the four neighbourhoods.  Eight sorted columns (min3 / med3 / max3) serve the four
//            pixels: the median of nine is med3(max3 of the lows, med3 of the mids, min3 of the highs), max / min of the eight from the side
//            columns' ends -- 14 three-operand instructions per pixel where a 19-exchange network and two 7-step reductions take 52.  The
//            test once in float64 (hot and cold exclude each other: lo <= hi), every product and sum rounded on its own.  The flags stay in
//            a lane's registers; the workgroup adds its two counts in LDS, lane 0 adds them to the caller's pair with ONE 64-bit atomic
//            (hot in the low word) whose return value is the workgroup's first slot of the coordinate list, and the flagged lanes take
//            their slots behind it from an LDS counter.  A workgroup that flags nothing issues no atomic at all.
// Global accesses are 16 bytes wide when both pointers are 16-byte aligned and W % 4 == 0, 8 bytes when they are 8-byte aligned (W is
// even and a lane's first column a multiple of four: every pair then lies in one row, 8-byte aligned), else 4 bytes.
#include "common.h"

#define BPC_T 256
#define BPC_TW YOND_BPC_TILE_W
#define BPC_TH YOND_BPC_TILE_H
#define BPC_LW (BPC_TW + 4)                 /* LDS row: the tile's columns x0 - 2 .. x0 + TW + 1 */
#define BPC_LH (BPC_TH + 4)
#define BPC_LANES_X (BPC_TW / 4)            /* lanes side by side, four pixels each */
#define BPC_LANES_Y (BPC_T / BPC_LANES_X)
#define BPC_ROWS (BPC_TH / BPC_LANES_Y)     /* rows a lane takes: ty, ty + LANES_Y, ... */

static_assert(BPC_TW % 4 == 0 && BPC_T % BPC_LANES_X == 0 && BPC_TH % BPC_LANES_Y == 0 && BPC_TH % 2 == 0, "tile: columns in fours, rows shared evenly");
static_assert(BPC_LW % 4 == 0, "16-byte LDS reads need a row of whole vectors");
static_assert(4 * BPC_ROWS <= 32, "a lane's flags are one 32-bit mask per kind");

// the same-colour clamp: i stays on its parity, within [i & 1, n - 2 + (i & 1)] (n even, >= 2; i >= -2)
__device__ __forceinline__ int bpc_clamp(int i, int n) {
    const int p = i & 1;
    return min(max(i, p), n - 2 + p);
}

// the three-operand instructions: v_min3_f32, v_max3_f32, v_med3_f32
__device__ __forceinline__ float bpc_min3(float a, float b, float c) { return fminf(fminf(a, b), c); }
__device__ __forceinline__ float bpc_max3(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }
__device__ __forceinline__ float bpc_med3(float a, float b, float c) { return __builtin_amdgcn_fmed3f(a, b, c); }

// one column of a 3x3 window (rows y - 2, y, y + 2), sorted.  Neighbouring same-colour pixels share two of their three columns, so a
// lane sorts eight columns for its four pixels.
struct BpcCol {
    float lo, mid, hi;
};
__device__ __forceinline__ BpcCol bpc_col(float a, float b, float c) { return BpcCol{bpc_min3(a, b, c), bpc_med3(a, b, c), bpc_max3(a, b, c)}; }

// median of nine from the three sorted columns: the median of (the largest low, the median mid, the smallest high)
__device__ __forceinline__ float bpc_median9(const BpcCol& l, const BpcCol& m, const BpcCol& r) {
    return bpc_med3(bpc_max3(l.lo, m.lo, r.lo), bpc_med3(l.mid, m.mid, r.mid), bpc_min3(l.hi, m.hi, r.hi));
}

// 0: neither, 1: hot, 2: cold -- c against the largest and the smallest of its eight neighbours, in float64.  beta1 * ref + beta2 is the
// one product that feeds a sum.  The build's -ffp-contract=off keeps the two apart; so that this does not rest on a flag (-ffp-contract=fast
// fuses in the back end whatever a pragma says, and this ROCm's __dmul_rn / __dadd_rn are plain operators), the product passes through an
// empty asm statement, which emits nothing and which no pass can look through.
__device__ __forceinline__ int bpc_flag(float c, float hi, float lo, double beta1, double beta2, double t2) {
    const bool hot = c > hi, cold = c < lo;
    const float ref = hot ? hi : lo;
    const double d = hot ? (double)c - (double)hi : (double)lo - (double)c;
    double prod = beta1 * (double)fmaxf(ref, 0.0f);
    asm volatile("" : "+v"(prod));
    const double var = prod + beta2;
    const double lhs = d * d, rhs = t2 * var;
    const bool out = lhs > rhs;
    return (hot && out) ? 1 : ((cold && out) ? 2 : 0);
}

__global__ __launch_bounds__(BPC_T) void bpc_list_kernel(const float* in, float* out, int H, int W, const int* __restrict__ points, int n) {
    const int i = blockIdx.x * BPC_T + threadIdx.x;
    if (i >= n) return;
    const int y = points[2 * (size_t)i], x = points[2 * (size_t)i + 1];
    if (y < 0 || y >= H || x < 0 || x >= W) return;
    float v[9];
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx)
            v[3 * (dy + 1) + dx + 1] = in[(size_t)bpc_clamp(y + 2 * dy, H) * W + bpc_clamp(x + 2 * dx, W)];
    out[(size_t)y * W + x] = bpc_median9(bpc_col(v[0], v[3], v[6]), bpc_col(v[1], v[4], v[7]), bpc_col(v[2], v[5], v[8]));
}

// VEC: floats per global access (4, 2 or 1)
template <int VEC>
__global__ __launch_bounds__(BPC_T) void bpc_detect_kernel(const float* __restrict__ in, float* __restrict__ out, int H, int W, double beta1,
                                                           double beta2, double t2, unsigned long long* __restrict__ counts,
                                                           int* __restrict__ coords, int cap) {
    __shared__ __attribute__((aligned(16))) float s_tile[BPC_LH][BPC_LW];
    __shared__ unsigned s_cnt[2], s_slot;
    __shared__ unsigned long long s_base;
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * BPC_TW, y0 = blockIdx.y * BPC_TH;
    if (tid < 2) s_cnt[tid] = 0;
    if (tid == 2) s_slot = 0;

    // stage: the tile's own columns in vectors (a vector that leaves the frame: element by element through the clamp), then the halo columns
    constexpr int VPR = BPC_TW / VEC;
    for (int i = tid; i < BPC_LH * VPR; i += BPC_T) {
        const int r = i / VPR, j = i - r * VPR;
        const int gy = bpc_clamp(y0 - 2 + r, H), gx = x0 + j * VEC;
        float* dst = &s_tile[r][2 + j * VEC];
        const float* row = in + (size_t)gy * W;
        if (gx + VEC <= W) {
            if constexpr (VEC == 4) {
                const f32x4 v = *(const f32x4*)(row + gx);
                *(f32x2*)dst = f32x2{v[0], v[1]};
                *(f32x2*)(dst + 2) = f32x2{v[2], v[3]};
            } else if constexpr (VEC == 2) {
                *(f32x2*)dst = *(const f32x2*)(row + gx);
            } else {
                *dst = row[gx];
            }
        } else {
#pragma unroll
            for (int e = 0; e < VEC; ++e) dst[e] = row[bpc_clamp(gx + e, W)];
        }
    }
    for (int i = tid; i < BPC_LH * 4; i += BPC_T) {
        const int r = i >> 2, k = i & 3;
        const int lx = k < 2 ? k : BPC_TW + k;
        s_tile[r][lx] = in[(size_t)bpc_clamp(y0 - 2 + r, H) * W + bpc_clamp(x0 - 2 + lx, W)];
    }
    __syncthreads();

    const int tx = tid % BPC_LANES_X, ty = tid / BPC_LANES_X;
    const int x = x0 + 4 * tx;
    unsigned hot_mask = 0, cold_mask = 0;                    // bit 4 * k + e: pixel e of the lane's row k
#pragma unroll
    for (int k = 0; k < BPC_ROWS; ++k) {
        const int oy = ty + k * BPC_LANES_Y, y = y0 + oy;
        if (y >= H || x >= W) continue;
        float a[3][8];                                       // LDS rows oy, oy + 2, oy + 4 are the frame's y - 2, y, y + 2; columns x - 2 .. x + 5
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const f32x4 u = *(const f32x4*)&s_tile[oy + 2 * r][4 * tx], w = *(const f32x4*)&s_tile[oy + 2 * r][4 * tx + 4];
            a[r][0] = u[0]; a[r][1] = u[1]; a[r][2] = u[2]; a[r][3] = u[3];
            a[r][4] = w[0]; a[r][5] = w[1]; a[r][6] = w[2]; a[r][7] = w[3];
        }
        BpcCol col[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) col[j] = bpc_col(a[0][j], a[1][j], a[2][j]);
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {                        // pixel e: columns e, e + 2 (its own), e + 4
            const float c = a[1][e + 2];
            const float m = bpc_median9(col[e], col[e + 2], col[e + 4]);
            // the eight without the centre: the side columns whole, of its own column the two ends
            const float hi = bpc_max3(col[e].hi, col[e + 4].hi, fmaxf(a[0][e + 2], a[2][e + 2]));
            const float lo = bpc_min3(col[e].lo, col[e + 4].lo, fminf(a[0][e + 2], a[2][e + 2]));
            const int f = x + e < W ? bpc_flag(c, hi, lo, beta1, beta2, t2) : 0;
            hot_mask |= (unsigned)(f == 1) << (4 * k + e);
            cold_mask |= (unsigned)(f == 2) << (4 * k + e);
            o[e] = f ? m : c;
        }
        float* dst = out + (size_t)y * W + x;
        if constexpr (VEC == 4) {
            *(f32x4*)dst = f32x4{o[0], o[1], o[2], o[3]};    // (W % 4 == 0: the four pixels are in the frame)
        } else if constexpr (VEC == 2) {
            *(f32x2*)dst = f32x2{o[0], o[1]};
            if (x + 2 < W) *(f32x2*)(dst + 2) = f32x2{o[2], o[3]};
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (x + e < W) dst[e] = o[e];
        }
    }

    // counts: a wave's sum by shuffles, the waves' through LDS, one global atomic of the workgroup for both counters
    int nh = __popc(hot_mask), nc = __popc(cold_mask);
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        nh += __shfl_xor(nh, s);
        nc += __shfl_xor(nc, s);
    }
    if ((tid & 63) == 0 && (nh | nc)) {
        atomicAdd(&s_cnt[0], (unsigned)nh);
        atomicAdd(&s_cnt[1], (unsigned)nc);
    }
    __syncthreads();
    const unsigned total = s_cnt[0] + s_cnt[1];
    if (total == 0) return;                                  // (uniform over the workgroup)
    if (tid == 0) s_base = atomicAdd(counts, ((unsigned long long)s_cnt[1] << 32) | s_cnt[0]);
    if (cap <= 0) return;                                    // (uniform: a kernel argument)
    __syncthreads();
    const unsigned long long before = s_base;
    const unsigned long long base = (before & 0xffffffffull) + (before >> 32);    // flagged before this workgroup's: its first slot
    if (base >= (unsigned long long)cap) return;
    unsigned mask = hot_mask | cold_mask;
    while (mask) {
        const int b = __ffs(mask) - 1;
        mask &= mask - 1;
        const unsigned long long slot = base + atomicAdd(&s_slot, 1u);
        if (slot < (unsigned long long)cap) {
            coords[2 * slot] = y0 + ty + (b >> 2) * BPC_LANES_Y;
            coords[2 * slot + 1] = x + (b & 3);
        }
    }
}

// H and W even and >= 2, H * W < 2^31
static int bpc_geometry(int H, int W) {
    if (H < 2 || W < 2 || (H & 1) || (W & 1)) return YOND_EINVAL;
    if ((unsigned long long)H * (unsigned long long)W >= (1ull << 31)) return YOND_EINVAL;
    return YOND_OK;
}

extern "C" int yond_bpc_repair_list_f32(const float* in, float* out, int H, int W, const int* points, int n, void* stream) {
    if (!in || !out || n < 0 || (n > 0 && !points)) return YOND_EINVAL;
    if (((((uintptr_t)in) | ((uintptr_t)out)) & 3u) || (((uintptr_t)points) & 3u)) return YOND_EINVAL;
    if (bpc_geometry(H, W) != YOND_OK) return YOND_EINVAL;
    if (out == in && n > 1) return YOND_EINVAL;              // a second point could read the first one's repair
    if (n == 0) return YOND_OK;
    hipLaunchKernelGGL(bpc_list_kernel, dim3(((unsigned)n + BPC_T - 1u) / BPC_T), dim3(BPC_T), 0, (hipStream_t)stream, in, out, H, W, points, n);
    YOND_LAUNCH_CHECK();
    return YOND_OK;
}

extern "C" int yond_bpc_detect_repair_f32(const float* in, float* out, int H, int W, double beta1, double beta2, double t, unsigned* counts,
                                          int* coords, int cap, void* stream) {
    if (!in || !out || !counts || out == in || cap < 0) return YOND_EINVAL;
    if ((((uintptr_t)in) | ((uintptr_t)out) | ((uintptr_t)coords)) & 3u) return YOND_EINVAL;
    if (((uintptr_t)counts) & 7u) return YOND_EINVAL;        // the pair is added to as one 64-bit word
    if (bpc_geometry(H, W) != YOND_OK) return YOND_EINVAL;
    const dim3 grid((unsigned)((W + BPC_TW - 1) / BPC_TW), (unsigned)((H + BPC_TH - 1) / BPC_TH));
    if (grid.y > 65535u) return YOND_EUNSUPPORTED;
    if (!coords) cap = 0;
    const uintptr_t both = ((uintptr_t)in) | ((uintptr_t)out);
    const double t2 = t * t;
    unsigned long long* pair = (unsigned long long*)counts;
    hipStream_t st = (hipStream_t)stream;
    if (!(both & 15u) && W % 4 == 0)
        hipLaunchKernelGGL(bpc_detect_kernel<4>, grid, dim3(BPC_T), 0, st, in, out, H, W, beta1, beta2, t2, pair, coords, cap);
    else if (!(both & 7u))
        hipLaunchKernelGGL(bpc_detect_kernel<2>, grid, dim3(BPC_T), 0, st, in, out, H, W, beta1, beta2, t2, pair, coords, cap);
    else
        hipLaunchKernelGGL(bpc_detect_kernel<1>, grid, dim3(BPC_T), 0, st, in, out, H, W, beta1, beta2, t2, pair, coords, cap);
    YOND_LAUNCH_CHECK();
    return YOND_OK;
}
