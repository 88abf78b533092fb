// The backward of FBI_Net (fbinet.hip) for the training step: what the inference kernels do not already give.  Activations and
// gradients are [N][H][W][nf] float32, nf = 32 or 64; every product is an exact fp32 product (the fp32-input MFMA; exact float64
// products of two float32 in the reductions; fmaf in the elementwise chains), no operand is rounded to half.
//
//   wgrad      dW_t[co][ci] = sum over n, y, x of dz[n,y,x,co] x[n, y + dy_t, x + dx_t, ci] for the LIVE taps of set 0 | 1 (| 2: a 1x1),
//              db[co] = sum dz -- the hot kernel, below
//   prelu      u = (a [+ b]) / div,  y = u > 0 ? u : s u  (s per channel or ONE slope): every PReLU of the net with the averaging node
//              in front of it; u, the PReLU's input, is stored for the backward (slopes may be negative: u is not recoverable from y)
//   prelu_bwd  du = dy (u > 0 ? 1 : s) / div,  ds = sum of dy u where u <= 0
//   first_bwd  the first layer (1 -> nf, 8 live taps read from the packed batch through fbi_first_kernel's index map): dW, db
//   out_bwd    the output layer: y = W f + b, optional sigmoid on y0, pred = y0 x + y1 | y0: df, dW, db from dpred
// The data gradient of a tap convolution is the forward kernel on flipped, transposed weights (the sets are point-symmetric).
//
// Every sum over pixels: each workgroup stores its partial sums into a workspace, a finish launch adds them in float64 in workgroup
// order.  No float atomics: two runs give the same bits.
#include "common.h"
#include "fbi_taps.h"

namespace {

constexpr int TR_MAX_WG = 1024;          // workgroups of a reducing launch = partial sums the finish adds per element
constexpr int TR_WG_ROWS = 4;            // wgrad: image rows per workgroup (more once TR_MAX_WG workgroups would not cover the batch)
constexpr int TR_PIX_PER_THREAD = 8;     // the streaming reductions: about this many pixels per thread below TR_MAX_WG workgroups

bool nf_ok(int nf) { return nf == 32 || nf == 64; }

int stream_wgs(size_t npix, int nf) {
    const size_t per = (size_t)(256 / (nf / 4)) * TR_PIX_PER_THREAD;
    const size_t n = (npix + per - 1) / per;
    return (int)(n < 1 ? 1 : n > (size_t)TR_MAX_WG ? (size_t)TR_MAX_WG : n);
}

int wgrad_rows(long long rows) {
    const long long need = (rows + TR_MAX_WG - 1) / TR_MAX_WG;
    return (int)(need > TR_WG_ROWS ? need : TR_WG_ROWS);
}

__device__ __forceinline__ size_t tr_mosaic_index(size_t n, int y, int x, int h, int w) {     // (fbinet.hip's mosaic_index)
    return ((n * h + (y >> 1)) * w + (x >> 1)) * 4 + 2 * (y & 1) + (x & 1);
}

// out[k] = float(sum over workgroups g = 0 .. nwg - 1, in that order, of part[g][k]) in float64
template <typename P>
__global__ __launch_bounds__(256) void tr_finish_kernel(const P* __restrict__ part, int nwg, size_t K, float* __restrict__ out) {
    const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= K) return;
    double s = 0.0;
    for (int g = 0; g < nwg; ++g) s += (double)part[(size_t)g * K + k];
    out[k] = (float)s;
}

// the one-slope form: the nf per-channel sums, then their sum in channel order
__global__ __launch_bounds__(64) void tr_finish_fold_kernel(const double* __restrict__ part, int nwg, int nf, float* __restrict__ out) {
    __shared__ double s[64];
    double a = 0.0;
    if ((int)threadIdx.x < nf)
        for (int g = 0; g < nwg; ++g) a += part[(size_t)g * nf + threadIdx.x];
    s[threadIdx.x] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int c = 0; c < nf; ++c) t += s[c];
        out[0] = (float)t;
    }
}

template <typename P>
int launch_finish(const P* part, int nwg, size_t K, float* out, hipStream_t st) {
    hipLaunchKernelGGL(tr_finish_kernel<P>, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, st, part, nwg, K, out);
    YOND_LAUNCH_CHECK();
    return YOND_OK;
}

// ------------------------------------------------------------------------------------------------------
// wgrad.  K of the MFMA = pixels: D[co][ci] += dz[p][co] x[p + d_t][ci], two pixels per 32x32x2 step (lane half h takes pixel 2 s + h),
// both operands one float per lane, contiguous over the 32 lanes of a half (128 bytes of one pixel's channels).  A workgroup walks
// TR_WG_ROWS image rows; its 4 waves split the (tap, 32 output channels) units round-robin -- nf 64, 9 taps: 18 units of two 32x32
// tiles, at most 5 per wave (160 accumulator registers) -- and every wave walks all the workgroup's pixels for its units.  Reads
// outside the frame are zero.  The unit (tap 0, co tile) also adds up its dz operand: the bias gradient.  Partials: the workgroup's
// taps * nf * nf + nf floats, accumulated in fp32 over rows * W pixels; the finish adds the workgroups in float64.
// ------------------------------------------------------------------------------------------------------
template <int SET, int NCT>
__global__ __launch_bounds__(256) void fbi_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dz, float* __restrict__ part,
                                                        int H, int W, int rows_per, long long rows) {
    using T = FbiTaps<SET>;
    constexpr int NT = T::N, NF = 32 * NCT, NU = NT * NCT, MAXU = (NU + 3) / 4, U = 8;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), li = lane & 31, lh = lane >> 5;
    f32x16 acc[MAXU][NCT];
#pragma unroll
    for (int j = 0; j < MAXU; ++j)
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[j][ct][r] = 0.0f;
    // this wave's units, slot j: unit 4 j + wave -> (tap, co tile) and the tap's offset, all wave-uniform scalars
    int ut[MAXU], ucot[MAXU], udy[MAXU], udx[MAXU];
#pragma unroll
    for (int j = 0; j < MAXU; ++j) ut[j] = -1;
    static_for<0, NU>([&](auto uc) {
        constexpr int unit = decltype(uc)::value, t = unit / NCT, j = unit / 4;
        if ((unit & 3) == wave) {
            ut[j] = t;
            ucot[j] = unit % NCT;
            udy[j] = (T::r[t] - T::K / 2) * T::DIL;
            udx[j] = (T::c[t] - T::K / 2) * T::DIL;
        }
    });
    float bs = 0.0f;                                                // (tap 0's units are 0 .. NCT - 1: slot 0 of waves 0 .. NCT - 1)
    const long long r0 = (long long)blockIdx.x * rows_per;
    const long long r1 = r0 + rows_per < rows ? r0 + rows_per : rows;
    for (long long row = r0; row < r1; ++row) {
        const int y = (int)(row % H);
        const float* dzrow = dz + (size_t)row * W * NF;
        for (int x0 = 0; x0 < W; x0 += 2 * U) {
#pragma unroll
            for (int j = 0; j < MAXU; ++j) {
                if (ut[j] < 0) continue;                            // (wave-uniform)
                const bool rowok = (unsigned)(y + udy[j]) < (unsigned)H;
                const size_t xrow = rowok ? (size_t)(row + udy[j]) * W : 0;   // (row + dy stays inside image n whenever rowok)
                float a[U], b[NCT][U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int px = x0 + 2 * u + lh, xx = px + udx[j];
                    a[u] = px < W ? dzrow[(size_t)px * NF + ucot[j] * 32 + li] : 0.0f;
                    const bool ok = rowok && px < W && (unsigned)xx < (unsigned)W;
#pragma unroll
                    for (int ct = 0; ct < NCT; ++ct) b[ct][u] = ok ? x[(xrow + (size_t)xx) * NF + ct * 32 + li] : 0.0f;
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (j == 0 && ut[0] == 0) bs += a[u];
#pragma unroll
                    for (int ct = 0; ct < NCT; ++ct) acc[j][ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], b[ct][u], acc[j][ct], 0, 0, 0);
                }
            }
        }
    }
    // D[co][ci]: the lane holds column ci = li, rows co = 8 g + 4 lh + e in register 4 g + e
    float* mine = part + (size_t)blockIdx.x * ((size_t)NT * NF * NF + NF);
#pragma unroll
    for (int j = 0; j < MAXU; ++j) {
        if (ut[j] < 0) continue;
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = ucot[j] * 32 + 8 * (r >> 2) + 4 * lh + (r & 3);
                mine[((size_t)ut[j] * NF + co) * NF + ct * 32 + li] = acc[j][ct][r];
            }
        if (j == 0 && ut[0] == 0) {
            const float both = bs + __shfl_xor(bs, 32);             // the two pixel parities
            if (lh == 0) mine[(size_t)NT * NF * NF + ucot[0] * 32 + li] = both;
        }
    }
}

// ------------------------------------------------------------------------------------------------------
// The streaming kernels: a thread owns four channels (one 16-byte access per tensor and pixel), 256 / (nf / 4) pixels per workgroup
// pass.  Reductions: float64 per thread, LDS, then one thread per output adds the workgroup's pixel rows in row order.
// ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fbi_prelu_kernel(const float* __restrict__ a, const float* __restrict__ b, float div,
                                                        const float* __restrict__ slope, int slope_n, int nf, size_t total4,
                                                        float* __restrict__ u_out, float* __restrict__ y) {
    const int c4 = nf / 4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (size_t)gridDim.x * 256) {
        const int c = (int)(i % c4) * 4;
        f32x4 s = {slope[0], slope[0], slope[0], slope[0]};         // (a parameter where it lies: no 16-byte alignment asked of it)
        if (slope_n != 1) s = f32x4{slope[c], slope[c + 1], slope[c + 2], slope[c + 3]};
        f32x4 v = *(const f32x4*)(a + i * 4);
        if (b) v = v + *(const f32x4*)(b + i * 4);
        f32x4 u, o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            u[e] = v[e] / div;
            o[e] = u[e] > 0.0f ? u[e] : u[e] * s[e];
        }
        if (u_out) *(f32x4*)(u_out + i * 4) = u;
        *(f32x4*)(y + i * 4) = o;
    }
}

// LDS [256][4] doubles -> thread t < nf adds the ppw pixel rows of channel t in row order
__device__ __forceinline__ void tr_store_partials4(double (*s)[4], const double a[4], int nf, double* __restrict__ dst) {
    const int c4 = nf / 4, ppw = 256 / c4, t = threadIdx.x;
    __syncthreads();                                                // (the previous pass's reads)
#pragma unroll
    for (int e = 0; e < 4; ++e) s[t][e] = a[e];
    __syncthreads();
    if (t < nf) {
        double acc = 0.0;
        for (int r = 0; r < ppw; ++r) acc += s[r * c4 + (t >> 2)][t & 3];
        dst[t] = acc;
    }
}

__global__ __launch_bounds__(256) void fbi_prelu_bwd_kernel(const float* __restrict__ u, const float* __restrict__ dy, float div,
                                                            const float* __restrict__ slope, int slope_n, int nf, size_t npix,
                                                            float* __restrict__ du, double* __restrict__ ws) {
    __shared__ double sh[256][4];
    const int c4 = nf / 4, ppw = 256 / c4;
    const int cl = threadIdx.x % c4, pr = threadIdx.x / c4;
    f32x4 s = {slope[0], slope[0], slope[0], slope[0]};
    if (slope_n != 1) s = f32x4{slope[cl * 4], slope[cl * 4 + 1], slope[cl * 4 + 2], slope[cl * 4 + 3]};
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (size_t p = (size_t)blockIdx.x * ppw + pr; p < npix; p += (size_t)gridDim.x * ppw) {
        const f32x4 uv = *(const f32x4*)(u + p * nf + cl * 4), g = *(const f32x4*)(dy + p * nf + cl * 4);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool pos = uv[e] > 0.0f;
            o[e] = (pos ? g[e] : g[e] * s[e]) / div;
            if (!pos) acc[e] += (double)g[e] * (double)uv[e];       // (exact product of two float32)
        }
        *(f32x4*)(du + p * nf + cl * 4) = o;
    }
    tr_store_partials4(sh, acc, nf, ws + (size_t)blockIdx.x * nf);
}

// first layer: dW[t][c] = sum dz[p][c] x(p + d_t), t = the 8 taps of the 3x3 without its centre in row-major order; row 8: db[c] = sum dz[p][c]
__global__ __launch_bounds__(256) void fbi_first_bwd_kernel(const float* __restrict__ x4, const float* __restrict__ dz, int h, int w, int nf,
                                                            size_t npix, double* __restrict__ ws) {
    __shared__ double sh[256][4];
    const int H = 2 * h, W = 2 * w, c4 = nf / 4, ppw = 256 / c4;
    const int cl = threadIdx.x % c4, pr = threadIdx.x / c4;
    double acc[9][4];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[t][e] = 0.0;
    for (size_t p = (size_t)blockIdx.x * ppw + pr; p < npix; p += (size_t)gridDim.x * ppw) {
        const int x = (int)(p % W);
        const size_t row = p / W;
        const int y = (int)(row % H);
        const size_t n = row / H;
        const f32x4 g = *(const f32x4*)(dz + p * nf + cl * 4);
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const int k = t < 4 ? t : t + 1;
            const int yy = y + k / 3 - 1, xx = x + k % 3 - 1;
            float val = 0.0f;
            if ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W) val = x4[tr_mosaic_index(n, yy, xx, h, w)];
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[t][e] += (double)g[e] * (double)val;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[8][e] += (double)g[e];
    }
#pragma unroll
    for (int t = 0; t < 9; ++t) tr_store_partials4(sh, acc[t], nf, ws + ((size_t)blockIdx.x * 9 + t) * nf);
}

// output layer.  The forward's own expression for y0 (fbi_out_kernel: fmaf chain over the lane's four channels, xor-shuffles over the
// nf / 4 lanes of the pixel) feeds the sigmoid's derivative.  Partials per workgroup: dW0 [NF], dW1 [NF], db0, db1.
template <int NF>
__global__ __launch_bounds__(256) void fbi_out_bwd_kernel(const float* __restrict__ f, const float* __restrict__ wgt, const float* __restrict__ b,
                                                          int oc, int use_sigmoid, float sv, const float* __restrict__ x4,
                                                          const float* __restrict__ dpred4, int h, int w, size_t npix,
                                                          float* __restrict__ df, double* __restrict__ ws) {
    constexpr int LPP = NF / 4, PPB = 256 / LPP;
    __shared__ double sh[256][10];
    const int part = threadIdx.x % LPP, sub = threadIdx.x / LPP;
    const int H = 2 * h, W = 2 * w;
    const f32x4 w0 = *(const f32x4*)(wgt + part * 4);
    f32x4 w1 = {0.0f, 0.0f, 0.0f, 0.0f};
    if (oc == 2) w1 = *(const f32x4*)(wgt + NF + part * 4);
    double acc[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const size_t nblk = (npix + PPB - 1) / PPB;
    for (size_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {   // (uniform trip count: every lane reaches the shuffles)
        const size_t p = blk * PPB + sub;
        const bool valid = p < npix;
        f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
        if (valid) v = *(const f32x4*)(f + p * NF + part * 4);
        float d0 = fmaf(v[3], w0[3], fmaf(v[2], w0[2], fmaf(v[1], w0[1], v[0] * w0[0])));
#pragma unroll
        for (int o = LPP / 2; o > 0; o >>= 1) d0 += __shfl_xor(d0, o);
        if (!valid) continue;
        const int x = (int)(p % W);
        const size_t row = p / W;
        const int y = (int)(row % H);
        const size_t at = tr_mosaic_index(row / H, y, x, h, w);
        const float g = dpred4[at];
        float g0 = oc == 2 ? g * x4[at] : g;                        // d pred / d y0 = x (res) | 1
        const float g1 = oc == 2 ? g : 0.0f;
        if (use_sigmoid) {
            const float sg = 1.0f / (1.0f + expf(-(d0 + b[0])));
            g0 = g0 * (sv * (sg * (1.0f - sg)));
        }
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            o[e] = fmaf(g1, w1[e], g0 * w0[e]);
            acc[e] += (double)g0 * (double)v[e];
            acc[4 + e] += (double)g1 * (double)v[e];
        }
        *(f32x4*)(df + p * NF + part * 4) = o;
        if (part == 0) {
            acc[8] += (double)g0;
            acc[9] += (double)g1;
        }
    }
#pragma unroll
    for (int e = 0; e < 10; ++e) sh[threadIdx.x][e] = acc[e];
    __syncthreads();
    const int t = threadIdx.x;
    double* dst = ws + (size_t)blockIdx.x * (2 * NF + 2);
    if (t < 2 * NF) {
        const int which = t / NF, ch = t % NF;
        double a = 0.0;
        for (int r = 0; r < PPB; ++r) a += sh[r * LPP + (ch >> 2)][which * 4 + (ch & 3)];
        dst[t] = a;
    } else if (t < 2 * NF + 2) {
        double a = 0.0;
        for (int r = 0; r < PPB; ++r) a += sh[r * LPP][8 + (t - 2 * NF)];
        dst[t] = a;
    }
}

bool aligned16(const void* p) { return ((unsigned long long)p & 15ull) == 0; }

size_t wgrad_part_floats(int set, int nf) { return (size_t)(set == 0 ? FbiTaps<0>::N : set == 1 ? FbiTaps<1>::N : FbiTaps<2>::N) * nf * nf + nf; }

}  // namespace

extern "C" int yond_fbi_wgrad_rows(int N, int H) {
    if (N < 1 || H < 1) return YOND_EINVAL;
    return wgrad_rows((long long)N * H);
}

extern "C" size_t yond_fbi_train_ws_bytes(int nf, int N, int H, int W) {
    if (!nf_ok(nf) || N < 1 || H < 1 || W < 1) return 0;
    const long long rows = (long long)N * H;
    const int rp = wgrad_rows(rows);
    const size_t wg = (size_t)((rows + rp - 1) / rp) * wgrad_part_floats(0, nf) * sizeof(float);
    const size_t st = (size_t)stream_wgs((size_t)rows * W, nf) * 9 * nf * sizeof(double);      // (first_bwd: the largest streaming need)
    return wg > st ? wg : st;
}

extern "C" int yond_fbi_wgrad_f32(const float* x, const float* dz, int set, int nf, int N, int H, int W, float* dwb, void* ws, size_t ws_bytes,
                                  void* stream) {
    if (!x || !dz || !dwb || !ws || !nf_ok(nf) || set < 0 || set > 2 || N < 1 || H < 1 || W < 1) return YOND_EINVAL;
    if (!aligned16(ws)) return YOND_EINVAL;
    const long long rows = (long long)N * H;
    const int rp = wgrad_rows(rows);
    const long long nwg = (rows + rp - 1) / rp;
    const size_t K = wgrad_part_floats(set, nf);
    if (ws_bytes < (size_t)nwg * K * sizeof(float)) return YOND_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    float* part = (float*)ws;
#define FBI_WG(S, C) hipLaunchKernelGGL((fbi_wgrad_kernel<S, C>), dim3((unsigned)nwg), dim3(256), 0, st, x, dz, part, H, W, rp, rows)
    if (set == 0) { if (nf == 32) FBI_WG(0, 1); else FBI_WG(0, 2); }
    else if (set == 1) { if (nf == 32) FBI_WG(1, 1); else FBI_WG(1, 2); }
    else { if (nf == 32) FBI_WG(2, 1); else FBI_WG(2, 2); }
#undef FBI_WG
    YOND_LAUNCH_CHECK();
    return launch_finish<float>(part, (int)nwg, K, dwb, st);
}

extern "C" int yond_fbi_prelu_f32(const float* a, const float* b, float div, const float* slope, int slope_n, int nf, size_t npix, float* u,
                                  float* y, void* stream) {
    if (!a || !slope || !y || !nf_ok(nf) || npix == 0 || (slope_n != 1 && slope_n != nf) || !(div >= 1.0f)) return YOND_EINVAL;
    if (!aligned16(a) || !aligned16(b) || !aligned16(u) || !aligned16(y)) return YOND_EINVAL;
    const size_t total4 = npix * (nf / 4);
    size_t nb = (total4 + 255) / 256;
    if (nb > 256 * 32) nb = 256 * 32;
    hipLaunchKernelGGL(fbi_prelu_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, a, b, div, slope, slope_n, nf, total4, u, y);
    YOND_LAUNCH_CHECK();
    return YOND_OK;
}

extern "C" int yond_fbi_prelu_bwd_f32(const float* u, const float* dy, float div, const float* slope, int slope_n, int nf, size_t npix,
                                      float* du, float* dslope, void* ws, size_t ws_bytes, void* stream) {
    if (!u || !dy || !slope || !du || !dslope || !ws || !nf_ok(nf) || npix == 0 || (slope_n != 1 && slope_n != nf) || !(div >= 1.0f))
        return YOND_EINVAL;
    if (!aligned16(u) || !aligned16(dy) || !aligned16(du) || !aligned16(ws)) return YOND_EINVAL;
    const int nwg = stream_wgs(npix, nf);
    if (ws_bytes < (size_t)nwg * nf * sizeof(double)) return YOND_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(fbi_prelu_bwd_kernel, dim3((unsigned)nwg), dim3(256), 0, st, u, dy, div, slope, slope_n, nf, npix, du, (double*)ws);
    YOND_LAUNCH_CHECK();
    if (slope_n == 1) {
        hipLaunchKernelGGL(tr_finish_fold_kernel, dim3(1), dim3(64), 0, st, (const double*)ws, nwg, nf, dslope);
        YOND_LAUNCH_CHECK();
        return YOND_OK;
    }
    return launch_finish<double>((const double*)ws, nwg, (size_t)nf, dslope, st);
}

extern "C" int yond_fbi_first_bwd_f32(const float* x4, const float* dz, int N, int h, int w, int nf, float* dwb, void* ws, size_t ws_bytes,
                                      void* stream) {
    if (!x4 || !dz || !dwb || !ws || !nf_ok(nf) || N < 1 || h < 1 || w < 1 || h > 0x3fffffff || w > 0x3fffffff) return YOND_EINVAL;
    if (!aligned16(dz) || !aligned16(ws)) return YOND_EINVAL;
    const size_t npix = (size_t)N * (2 * (size_t)h) * (2 * (size_t)w);
    const int nwg = stream_wgs(npix, nf);
    if (ws_bytes < (size_t)nwg * 9 * nf * sizeof(double)) return YOND_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(fbi_first_bwd_kernel, dim3((unsigned)nwg), dim3(256), 0, st, x4, dz, h, w, nf, npix, (double*)ws);
    YOND_LAUNCH_CHECK();
    return launch_finish<double>((const double*)ws, nwg, (size_t)9 * nf, dwb, st);
}

extern "C" int yond_fbi_out_bwd_f32(const float* f, int nf, const float* w, const float* b, int oc, int use_sigmoid, float sigmoid_value,
                                    const float* x4, const float* dpred4, int N, int h, int wd, float* df, float* dwb, void* ws, size_t ws_bytes,
                                    void* stream) {
    if (!f || !w || !b || !dpred4 || !df || !dwb || !ws || !nf_ok(nf) || N < 1 || h < 1 || wd < 1) return YOND_EINVAL;
    if ((oc != 1 && oc != 2) || (oc == 2 && !x4) || (use_sigmoid != 0 && use_sigmoid != 1) || h > 0x3fffffff || wd > 0x3fffffff) return YOND_EINVAL;
    if (!aligned16(f) || !aligned16(w) || !aligned16(df) || !aligned16(ws)) return YOND_EINVAL;
    const size_t npix = (size_t)N * (2 * (size_t)h) * (2 * (size_t)wd);
    const int nwg = stream_wgs(npix, nf);
    const size_t K = 2 * (size_t)nf + 2;
    if (ws_bytes < (size_t)nwg * K * sizeof(double)) return YOND_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (nf == 32) hipLaunchKernelGGL(fbi_out_bwd_kernel<32>, dim3((unsigned)nwg), dim3(256), 0, st, f, w, b, oc, use_sigmoid, sigmoid_value, x4, dpred4, h, wd, npix, df, (double*)ws);
    else hipLaunchKernelGGL(fbi_out_bwd_kernel<64>, dim3((unsigned)nwg), dim3(256), 0, st, f, w, b, oc, use_sigmoid, sigmoid_value, x4, dpred4, h, wd, npix, df, (double*)ws);
    YOND_LAUNCH_CHECK();
    return launch_finish<double>((const double*)ws, nwg, K, dwb, st);
}
