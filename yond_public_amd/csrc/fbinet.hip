// FBI_Net (the reference's archs/comp.py:264-648, case 'FBI_Net'): a blind-spot denoiser on the full-resolution one-channel Bayer
// mosaic.  Activations are [N][H][W][nf] float32, nf = 32 or 64; every product is an exact fp32 product on the fp32-input MFMA
// (v_mfma_f32_32x32x2_f32: bit for bit a chain of fused multiply-adds) or, in the two edge kernels, a plain fmaf.  No operand is
// rounded to half: no range precondition, no status word.
//
//   first    packed Bayer [N][h][w][4] -> n = PReLU(conv3x3 without its centre tap (x) + b; one slope)          bound by its stores
//   tapconv  n' = PReLU(sum over the LIVE taps of W_t n(. + d_t) + b; s1),  o' = PReLU((n' + o) / 2; s2)         the hot kernel
//   rm       o = PReLU((v + W2 PReLU(W1 v + b1; a1) + b2) / 2; a2),  sum = o  or  sum += o                       two chained 1x1 GEMMs
//   out      y = W f + b (nf -> 1 | 2), optional sigmoid on y0, a x + b or y -> packed Bayer [N][h][w][4]        bound by its loads
//
// MFMA orientation in tapconv and rm: D = W . X^T -- the A operand is a weight column (row = output channel), the B operand a pixel
// column (column = pixel), so a lane ends with 16 output channels of ONE pixel, c = 8 g + 4 (lane >> 5) + e for register 4 g + e:
// four 16-byte stores per 32 channels.  The k index of a step is free as long as both operands agree: lane half h of step (g, e) takes
// channel 8 g + 4 h + e, so a lane's four consecutive steps read ONE 16-byte slot of its pixel -- and an accumulator tile is, as it
// stands, the B operand of the next product over its channels (rm chains its two GEMMs without LDS or lane movement).
#include "common.h"
#include "fbi_taps.h"

#define FBI_TH 8        // tapconv's pixel tile: 8 rows (two per wave) x 32 columns (the MFMA's 32 columns)
#define FBI_TW 32

__device__ __forceinline__ float prelu_f(float x, float s) { return x > 0.0f ? x : x * s; }

// ------------------------------------------------------------------------------------------------------
// tapconv.  One workgroup: 8 x 32 output pixels, all nf output channels; the input tile with its halo goes through LDS in chunks
// of 16 input channels (pixel stride 20 floats: a 16-byte read per lane, half h of the wave 16 bytes further; the next chunk travels
// from global memory to registers under this chunk's products), the live taps' weights come packed, 16 bytes per lane and four
// k-steps, straight from global memory (the four waves read the same lines).  A frame smaller than the tile or than the halo is one
// partly filled tile: what lies outside is zero on the way in and not stored on the way out.
// ------------------------------------------------------------------------------------------------------
template <int SET, int NCT>
__global__ __launch_bounds__(256) void fbi_tapconv_kernel(const float* __restrict__ n_in, const float* __restrict__ o_in,
                                                          const float* __restrict__ wpk, const float* __restrict__ bias,
                                                          const float* __restrict__ s1, const float* __restrict__ s2,
                                                          float* __restrict__ n_out, float* __restrict__ o_out, int H, int W) {
    using T = FbiTaps<SET>;
    constexpr int NT = T::N, HALO = T::HALO, NF = 32 * NCT, KC = 16, KCP = 20, MW = FBI_TH / 4;
    constexpr int IH = FBI_TH + 2 * HALO, IW = FBI_TW + 2 * HALO;
    __shared__ __attribute__((aligned(16))) float s_in[IH * IW * KCP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, lh = lane >> 5;
    const int ntx = (W + FBI_TW - 1) / FBI_TW;
    const int tx = blockIdx.x % ntx, ty = blockIdx.x / ntx, n = blockIdx.y;
    const int ox0 = tx * FBI_TW, oy0 = ty * FBI_TH;
    const size_t img = (size_t)n * H * W;

    f32x16 acc[MW][NCT];
#pragma unroll
    for (int m = 0; m < MW; ++m)
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][ct][r] = 0.0f;

    // the next chunk's tile is on its way from global memory to registers while this chunk's products run
    constexpr int NLD = (IH * IW * 4 + 255) / 256;
    f32x4 pre[NLD];
    auto gload = [&](int chunk) {
#pragma unroll
        for (int j = 0; j < NLD; ++j) {
            const int it = tid + j * 256;
            const int pix = it >> 2, part = it & 3;
            const int py = pix / IW, px = pix - py * IW;
            const int gy = oy0 - HALO + py, gx = ox0 - HALO + px;
            f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};                     // the zero border (padding = HALO, zeros)
            if (it < IH * IW * 4 && (unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W)
                v = *(const f32x4*)(n_in + (img + (size_t)gy * W + gx) * NF + chunk * KC + part * 4);
            pre[j] = v;
        }
    };
    gload(0);
    for (int chunk = 0; chunk < NF / KC; ++chunk) {
        __syncthreads();                                            // (the previous chunk's reads are done)
#pragma unroll
        for (int j = 0; j < NLD; ++j) {
            const int it = tid + j * 256;
            if (it < IH * IW * 4) *(f32x4*)(s_in + (it >> 2) * KCP + (it & 3) * 4) = pre[j];
        }
        __syncthreads();
        if (chunk + 1 < NF / KC) gload(chunk + 1);
        static_for<0, NT>([&](auto tc) {
            constexpr int t = decltype(tc)::value;
            constexpr int dy = (T::r[t] - T::K / 2) * T::DIL, dx = (T::c[t] - T::K / 2) * T::DIL;
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                f32x4 wv[NCT];
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct)
                    wv[ct] = *(const f32x4*)(wpk + ((size_t)(((chunk * NT + t) * 2 + q) * NCT + ct) * 64 + lane) * 4);
#pragma unroll
                for (int m = 0; m < MW; ++m) {
                    const f32x4 b = *(const f32x4*)(s_in + ((wave * MW + m + HALO + dy) * IW + li + HALO + dx) * KCP + q * 8 + lh * 4);
#pragma unroll
                    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            acc[m][ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[ct][e], b[e], acc[m][ct], 0, 0, 0);   // D = W . X^T
                }
            }
        });
    }

    const int ox = ox0 + li;
#pragma unroll
    for (int m = 0; m < MW; ++m) {
        const int oy = oy0 + wave * MW + m;
        if (oy >= H || ox >= W) continue;
        const size_t base = (img + (size_t)oy * W + ox) * NF;
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int c = ct * 32 + 8 * g + 4 * lh;
                const f32x4 bv = *(const f32x4*)(bias + c), a1 = *(const f32x4*)(s1 + c), a2 = *(const f32x4*)(s2 + c);
                const f32x4 ov = *(const f32x4*)(o_in + base + c);
                f32x4 nv, rv;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    nv[e] = prelu_f(acc[m][ct][4 * g + e] + bv[e], a1[e]);
                    rv[e] = prelu_f((nv[e] + ov[e]) * 0.5f, a2[e]);
                }
                *(f32x4*)(n_out + base + c) = nv;
                *(f32x4*)(o_out + base + c) = rv;
            }
    }
}

// w: OIHW [nf][nf][k][k] (k = 5 for set 0, 3 for set 1), unmasked: only the live taps are read.  dst: taps * nf * nf floats,
// [chunk of 16 input channels][tap][q][32 output channels tile][lane][e]:  co = 32 ct + (lane & 31),  ci = 16 chunk + 8 q + 4 (lane >> 5) + e
template <int SET>
static void pack_tap(const float* w, int nf, float* dst) {
    using T = FbiTaps<SET>;
    size_t o = 0;
    for (int chunk = 0; chunk < nf / 16; ++chunk)
        for (int t = 0; t < T::N; ++t)
            for (int q = 0; q < 2; ++q)
                for (int ct = 0; ct < nf / 32; ++ct)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int e = 0; e < 4; ++e) {
                            const int co = ct * 32 + (lane & 31), ci = chunk * 16 + q * 8 + (lane >> 5) * 4 + e;
                            dst[o++] = w[(((size_t)co * nf + ci) * T::K + T::r[t]) * T::K + T::c[t]];
                        }
}

extern "C" int yond_fbi_taps(int set) { return set == 0 ? FbiTaps<0>::N : set == 1 ? FbiTaps<1>::N : YOND_EINVAL; }

extern "C" int yond_fbi_tile(int* th, int* tw) {
    if (!th || !tw) return YOND_EINVAL;
    *th = FBI_TH;
    *tw = FBI_TW;
    return YOND_OK;
}

extern "C" int yond_pack_fbi_tap_weight_f32(const float* w, int nf, int set, float* dst) {
    if (!w || !dst || (nf != 32 && nf != 64) || (set != 0 && set != 1)) return YOND_EINVAL;
    if (set == 0) pack_tap<0>(w, nf, dst); else pack_tap<1>(w, nf, dst);
    return YOND_OK;
}

extern "C" int yond_fbi_tapconv_f32(const float* n_in, const float* o_in, int set, int nf, const float* wpk, const float* bias,
                                    const float* s1, const float* s2, int N, int H, int W, float* n_out, float* o_out, void* stream) {
    if (!n_in || !o_in || !wpk || !bias || !s1 || !s2 || !n_out || !o_out) return YOND_EINVAL;
    if (n_out == n_in || o_out == n_in) return YOND_EINVAL;       // (the tile's halo is read after other tiles have stored)
    if ((nf != 32 && nf != 64) || (set != 0 && set != 1) || N < 1 || N > 65535 || H < 1 || W < 1) return YOND_EINVAL;
    const long long tiles = (long long)((W + FBI_TW - 1) / FBI_TW) * ((H + FBI_TH - 1) / FBI_TH);
    if (tiles > 0x7fffffffLL) return YOND_EINVAL;
    const dim3 grid((unsigned)tiles, (unsigned)N), block(256);
    hipStream_t st = (hipStream_t)stream;
#define FBI_TAP(S, C) hipLaunchKernelGGL((fbi_tapconv_kernel<S, C>), grid, block, 0, st, n_in, o_in, wpk, bias, s1, s2, n_out, o_out, H, W)
    if (set == 0) { if (nf == 32) FBI_TAP(0, 1); else FBI_TAP(0, 2); }
    else { if (nf == 32) FBI_TAP(1, 1); else FBI_TAP(1, 2); }
#undef FBI_TAP
    YOND_LAUNCH_CHECK();
    return YOND_OK;
}

// ------------------------------------------------------------------------------------------------------
// rm: the residual module (archs/comp.py:303-322) on 32 pixels per wave.  v is loaded in the accumulator layout (a lane: its pixel's
// channels 8 g + 4 h + e), which is also the B operand's; W1 v accumulates in the same layout, gets its bias and PReLU in registers
// and is the B operand of W2.  Both packed weights (2 nf^2 floats, 32 KB at nf 64) sit in LDS for the workgroup's life.
//   pre_slope != NULL: v = PReLU(v / pre_div; pre_slope) first (the network's tail: output_sum / num_of_layers, :622).
//   sum_mode 0: sum untouched, 1: sum = o, 2: sum += o.
// ------------------------------------------------------------------------------------------------------
template <int NCT>
__global__ __launch_bounds__(256) void fbi_rm_kernel(const float* __restrict__ v_in, const float* __restrict__ w1p,
                                                     const float* __restrict__ b1, const float* __restrict__ a1,
                                                     const float* __restrict__ w2p, const float* __restrict__ b2,
                                                     const float* __restrict__ a2, const float* __restrict__ pre_slope, float pre_div,
                                                     float* __restrict__ o_out, float* sum, int sum_mode, size_t npix) {
    constexpr int NF = 32 * NCT;
    __shared__ __attribute__((aligned(16))) float s_w[2 * NF * NF];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, lh = lane >> 5;
    for (int it = tid; it < NF * NF / 4; it += 256) {
        *(f32x4*)(s_w + it * 4) = *(const f32x4*)(w1p + it * 4);
        *(f32x4*)(s_w + NF * NF + it * 4) = *(const f32x4*)(w2p + it * 4);
    }
    __syncthreads();
    const size_t ntiles = (npix + 31) / 32, tstep = (size_t)gridDim.x * 4;
    // the next tile's pixels are loaded before this tile's products start (the wave is alone on its SIMD: the packed weights, which the
    // compiler keeps in registers across the loop, leave room for one wave)
    f32x4 nxt[NCT][4];
    auto vload = [&](size_t tile) {
        const size_t p = tile * 32 + li;
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f32x4 x = {0.0f, 0.0f, 0.0f, 0.0f};
                if (tile < ntiles && p < npix) x = *(const f32x4*)(v_in + p * NF + ct * 32 + 8 * g + 4 * lh);
                nxt[ct][g] = x;
            }
    };
    vload((size_t)blockIdx.x * 4 + wave);
    for (size_t tile = (size_t)blockIdx.x * 4 + wave; tile < ntiles; tile += tstep) {
        const size_t p = tile * 32 + li;
        const bool valid = p < npix;
        f32x4 v[NCT][4];
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
            for (int g = 0; g < 4; ++g) v[ct][g] = nxt[ct][g];
        vload(tile + tstep);
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int c = ct * 32 + 8 * g + 4 * lh;
                f32x4 x = v[ct][g];
                if (pre_slope) {
                    const f32x4 ps = *(const f32x4*)(pre_slope + c);
#pragma unroll
                    for (int e = 0; e < 4; ++e) x[e] = prelu_f(x[e] / pre_div, ps[e]);
                }
                v[ct][g] = x;
            }
        f32x16 h[NCT];
#pragma unroll
        for (int co = 0; co < NCT; ++co) {
#pragma unroll
            for (int r = 0; r < 16; ++r) h[co][r] = 0.0f;
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 wv = *(const f32x4*)(s_w + (((co * NCT + ct) * 4 + g) * 64 + lane) * 4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) h[co] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[e], v[ct][g][e], h[co], 0, 0, 0);
                }
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int c = co * 32 + 8 * g + 4 * lh;
                const f32x4 bv = *(const f32x4*)(b1 + c), av = *(const f32x4*)(a1 + c);
#pragma unroll
                for (int e = 0; e < 4; ++e) h[co][4 * g + e] = prelu_f(h[co][4 * g + e] + bv[e], av[e]);
            }
        }
#pragma unroll
        for (int co = 0; co < NCT; ++co) {
            f32x16 r2;
#pragma unroll
            for (int r = 0; r < 16; ++r) r2[r] = 0.0f;
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 wv = *(const f32x4*)(s_w + NF * NF + (((co * NCT + ct) * 4 + g) * 64 + lane) * 4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) r2 = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[e], h[ct][4 * g + e], r2, 0, 0, 0);
                }
            if (!valid) continue;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int c = co * 32 + 8 * g + 4 * lh;
                const f32x4 bv = *(const f32x4*)(b2 + c), av = *(const f32x4*)(a2 + c);
                f32x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = prelu_f((v[co][g][e] + (r2[4 * g + e] + bv[e])) * 0.5f, av[e]);
                if (o_out) *(f32x4*)(o_out + p * NF + c) = o;
                if (sum_mode == 1) *(f32x4*)(sum + p * NF + c) = o;
                else if (sum_mode == 2) {
                    const f32x4 s = *(const f32x4*)(sum + p * NF + c);
                    *(f32x4*)(sum + p * NF + c) = s + o;
                }
            }
        }
    }
}

// w: [nf][nf] (a 1x1 convolution's OI11) -> [32 outputs tile][32 inputs tile][g][lane][e]:  co = 32 cot + (lane & 31),  ci = 32 ct + 8 g + 4 (lane >> 5) + e
extern "C" int yond_pack_fbi_rm_weight_f32(const float* w, int nf, float* dst) {
    if (!w || !dst || (nf != 32 && nf != 64)) return YOND_EINVAL;
    size_t o = 0;
    for (int cot = 0; cot < nf / 32; ++cot)
        for (int ct = 0; ct < nf / 32; ++ct)
            for (int g = 0; g < 4; ++g)
                for (int lane = 0; lane < 64; ++lane)
                    for (int e = 0; e < 4; ++e)
                        dst[o++] = w[(size_t)(cot * 32 + (lane & 31)) * nf + ct * 32 + 8 * g + 4 * (lane >> 5) + e];
    return YOND_OK;
}

extern "C" int yond_fbi_rm_f32(const float* v, int nf, const float* w1p, const float* b1, const float* a1, const float* w2p, const float* b2,
                               const float* a2, const float* pre_slope, int pre_div, size_t npix, float* o_out, float* sum, int sum_mode,
                               void* stream) {
    if (!v || !w1p || !b1 || !a1 || !w2p || !b2 || !a2 || npix == 0 || (nf != 32 && nf != 64)) return YOND_EINVAL;
    if (sum_mode < 0 || sum_mode > 2 || (sum_mode != 0 && !sum) || (sum_mode == 0 && !o_out)) return YOND_EINVAL;
    if (pre_slope && pre_div < 1) return YOND_EINVAL;
    size_t nb = ((npix + 31) / 32 + 3) / 4;
    if (nb > 1024) nb = 1024;                                    // every workgroup copies the weights to LDS once: few, long-lived
    hipStream_t st = (hipStream_t)stream;
    if (nf == 32) hipLaunchKernelGGL(fbi_rm_kernel<1>, dim3((unsigned)nb), dim3(256), 0, st, v, w1p, b1, a1, w2p, b2, a2, pre_slope, (float)pre_div, o_out, sum, sum_mode, npix);
    else hipLaunchKernelGGL(fbi_rm_kernel<2>, dim3((unsigned)nb), dim3(256), 0, st, v, w1p, b1, a1, w2p, b2, a2, pre_slope, (float)pre_div, o_out, sum, sum_mode, npix);
    YOND_LAUNCH_CHECK();
    return YOND_OK;
}

// ------------------------------------------------------------------------------------------------------
// first (archs/comp.py:264-275, 389-395): 1 -> nf, 3x3 without its centre.  The mosaic pixel (y, x) is element 2 (y & 1) + (x & 1) of
// the packed pixel (y / 2, x / 2): the index map is done here, there is no layout copy.  One thread: 4 output channels of one pixel
// (nf / 4 neighbouring threads share the pixel: its 16-byte stores are contiguous across them).
// ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ size_t mosaic_index(size_t n, int y, int x, int h, int w) {
    return ((n * h + (y >> 1)) * w + (x >> 1)) * 4 + 2 * (y & 1) + (x & 1);
}

__global__ __launch_bounds__(256) void fbi_first_kernel(const float* __restrict__ x4, const float* __restrict__ wpk,
                                                        const float* __restrict__ bias, const float* __restrict__ slope,
                                                        float* __restrict__ dst, int h, int w, int nf, size_t total) {
    const int H = 2 * h, W = 2 * w, ng = nf / 4;
    const float s = slope[0];
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        const int cg = (int)(idx % ng);
        const size_t pix = idx / ng;
        const int x = (int)(pix % W);
        const size_t row = pix / W;
        const int y = (int)(row % H);
        const size_t n = row / H;
        f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const int k = t < 4 ? t : t + 1;                        // the 3x3 taps in row-major order without the centre
            const int yy = y + k / 3 - 1, xx = x + k % 3 - 1;
            float val = 0.0f;
            if ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W) val = x4[mosaic_index(n, yy, xx, h, w)];
            const f32x4 wv = *(const f32x4*)(wpk + t * nf + cg * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = fmaf(val, wv[e], acc[e]);
        }
        const f32x4 bv = *(const f32x4*)(bias + cg * 4);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = prelu_f(acc[e] + bv[e], s);
        *(f32x4*)(dst + pix * nf + cg * 4) = o;
    }
}

// w: [nf][1][3][3] -> [8 live taps][nf]
extern "C" int yond_pack_fbi_first_weight_f32(const float* w, int nf, float* dst) {
    if (!w || !dst || (nf != 32 && nf != 64)) return YOND_EINVAL;
    for (int t = 0; t < 8; ++t)
        for (int co = 0; co < nf; ++co) dst[t * nf + co] = w[co * 9 + (t < 4 ? t : t + 1)];
    return YOND_OK;
}

static unsigned fbi_grid(size_t total, size_t per_block) {
    size_t nb = (total + per_block - 1) / per_block;
    if (nb > 256 * 32) nb = 256 * 32;
    return (unsigned)(nb < 1 ? 1 : nb);
}

extern "C" int yond_fbi_first_f32(const float* x4, int N, int h, int w, int nf, const float* wpk, const float* bias, const float* slope,
                                  float* dst, void* stream) {
    if (!x4 || !wpk || !bias || !slope || !dst || N < 1 || h < 1 || w < 1 || (nf != 32 && nf != 64)) return YOND_EINVAL;
    if (h > 0x3fffffff || w > 0x3fffffff) return YOND_EINVAL;
    const size_t total = (size_t)N * (2 * (size_t)h) * (2 * (size_t)w) * (nf / 4);
    hipLaunchKernelGGL(fbi_first_kernel, dim3(fbi_grid(total, 256)), dim3(256), 0, (hipStream_t)stream, x4, wpk, bias, slope, dst, h, w, nf, total);
    YOND_LAUNCH_CHECK();
    return YOND_OK;
}

// ------------------------------------------------------------------------------------------------------
// out (archs/comp.py:598, 624, 642-646): y = W f + b with 1 or 2 outputs; y0 = sigmoid_value * sigmoid(y0) if asked;
// 2 outputs: dst = y0 * x + y1 (`res`), 1 output: dst = y0.  nf / 4 lanes share a pixel (16 bytes of it each: a wave reads
// contiguous memory) and combine their partial sums by xor-shuffles; the result goes to the packed Bayer position.
// ------------------------------------------------------------------------------------------------------
template <int NF>
__global__ __launch_bounds__(256) void fbi_out_kernel(const float* __restrict__ f, const float* __restrict__ wgt, const float* __restrict__ b,
                                                      int oc, int use_sigmoid, float sv, const float* __restrict__ x4,
                                                      float* __restrict__ dst4, int h, int w, size_t npix) {
    constexpr int LPP = NF / 4, PPB = 256 / LPP;
    const int part = threadIdx.x % LPP, sub = threadIdx.x / LPP;
    const int H = 2 * h, W = 2 * w;
    const f32x4 w0 = *(const f32x4*)(wgt + part * 4);
    f32x4 w1 = {0.0f, 0.0f, 0.0f, 0.0f};
    if (oc == 2) w1 = *(const f32x4*)(wgt + NF + part * 4);
    const size_t nblk = (npix + PPB - 1) / PPB;
    for (size_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {   // (uniform trip count: every lane reaches the shuffles)
        const size_t p = blk * PPB + sub;
        const bool valid = p < npix;
        f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
        if (valid) v = *(const f32x4*)(f + p * NF + part * 4);
        float d0 = fmaf(v[3], w0[3], fmaf(v[2], w0[2], fmaf(v[1], w0[1], v[0] * w0[0])));
        float d1 = fmaf(v[3], w1[3], fmaf(v[2], w1[2], fmaf(v[1], w1[1], v[0] * w1[0])));
#pragma unroll
        for (int o = LPP / 2; o > 0; o >>= 1) {
            d0 += __shfl_xor(d0, o);
            d1 += __shfl_xor(d1, o);
        }
        if (!valid || part != 0) continue;
        const int x = (int)(p % W);
        const size_t row = p / W;
        const int y = (int)(row % H);
        const size_t at = mosaic_index(row / H, y, x, h, w);
        float y0 = d0 + b[0];
        if (use_sigmoid) y0 = sv * (1.0f / (1.0f + expf(-y0)));
        dst4[at] = oc == 2 ? fmaf(y0, x4[at], d1 + b[1]) : y0;
    }
}

extern "C" int yond_fbi_out_f32(const float* f, int nf, const float* w, const float* b, int oc, int use_sigmoid, float sigmoid_value,
                                const float* x4, int N, int h, int wd, float* dst4, void* stream) {
    if (!f || !w || !b || !dst4 || N < 1 || h < 1 || wd < 1 || (nf != 32 && nf != 64)) return YOND_EINVAL;
    if ((oc != 1 && oc != 2) || (oc == 2 && !x4) || (use_sigmoid != 0 && use_sigmoid != 1)) return YOND_EINVAL;
    if (h > 0x3fffffff || wd > 0x3fffffff) return YOND_EINVAL;
    const size_t npix = (size_t)N * (2 * (size_t)h) * (2 * (size_t)wd);
    hipStream_t st = (hipStream_t)stream;
    if (nf == 32) hipLaunchKernelGGL(fbi_out_kernel<32>, dim3(fbi_grid(npix, 32)), dim3(256), 0, st, f, w, b, oc, use_sigmoid, sigmoid_value, x4, dst4, h, wd, npix);
    else hipLaunchKernelGGL(fbi_out_kernel<64>, dim3(fbi_grid(npix, 16)), dim3(256), 0, st, f, w, b, oc, use_sigmoid, sigmoid_value, x4, dst4, h, wd, npix);
    YOND_LAUNCH_CHECK();
    return YOND_OK;
}
