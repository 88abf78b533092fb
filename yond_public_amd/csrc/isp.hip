// R1: raw Bayer frame -> sRGB on the device (utils/sidd_utils.py:156-277 process_sidd_image, utils/isp_ops.py:171-197 FastISP):
// clip, white balance, 14-bit quantisation, edge-aware demosaic, colour matrix, gamma, 8-bit codes (or float32 values).
//
// Memory bound (4 B in, 3 B out per pixel in codes form), so:
//   - a workgroup renders a 16 x 128 tile; its 18 x 136 quantised integers (one-pixel halo, rounded out to whole 16-byte groups) go
//     through LDS once: every input pixel is loaded as part of a float4 row load and quantised once;
//   - a thread owns a 2 x 4 strip (one RGGB quad row twice over): the four CFA sites are handled together, straight-line, no branch
//     by site; it reads its 4 x 6 neighbourhood with one ds_read_b128 + two ds_read_b32 per row;
//   - the strip's codes leave as two 12-byte stores (4 pixels x 3 channels), consecutive lanes on consecutive addresses;
//   - gamma: no per-element pow in the codes form.  code = #{k : t_k <= x} with the 255 float64 thresholds t_k = (k/255)^2.2 of
//     the host in LDS; a float32 exp2/log2 guess lands on the code or next to it and two table reads settle it exactly.
// Arithmetic contract (include/yond_hip.h): the reference's float64 steps in its order; no FMA contraction (-ffp-contract=off).
#include "common.h"

#define ISP_TH 16                    // tile rows
#define ISP_TW 128                   // tile columns
#define ISP_LW (ISP_TW + 8)          // LDS row: columns x0 - 4 .. x0 + TW + 3 (whole float4 groups of the frame)
#define ISP_LH (ISP_TH + 2)          // rows y0 - 1 .. y0 + TH

struct IspParams {
    double gain[4];                  // per CFA site (2 * (y & 1) + (x & 1) of the RGGB frame)
    double m[9];                     // colour matrix, row-major
    double inv_gamma;                // float form
    int H, W, flip_lr, flip_ud, layout, mode, order;
};

struct __attribute__((packed, aligned(4))) IspRgb4 { uint32_t w[3]; };      // four interleaved u8 pixels

// mirror without repeating the edge (-1 -> 1, n -> n - 2): keeps the CFA parity
__device__ __forceinline__ int isp_mirror(int v, int n) { return v < 0 ? -v : (v >= n ? 2 * n - 2 - v : v); }

// element offset of the RGGB frame's pixel (y, x) in the input
__device__ __forceinline__ size_t isp_src(const IspParams& p, int y, int x) {
    if (p.layout == YOND_ISP_PACKED4) return (((size_t)(y >> 1) * (p.W >> 1) + (x >> 1)) << 2) + ((y & 1) << 1) + (x & 1);
    return (size_t)(p.flip_ud ? p.H - 1 - y : y) * p.W + (p.flip_lr ? p.W - 1 - x : x);
}

// gains, clip, 14-bit quantisation of one input value at CFA site s
__device__ __forceinline__ int isp_quant(const IspParams& p, float v, int s) {
    if (p.mode == YOND_ISP_SIDD) {
        v = fminf(fmaxf(v, 0.0f), 1.0f);                                        // image.clip(0, 1)   (sidd_utils.py:158)
        double d = (double)v * p.gain[s];                                       // apply_gains: float32 x float64
        d = fmin(fmax(d, 0.0), 1.0);
        d = fmin(fmax(d * 16383.0, 0.0), 16383.0);                              // demosaic_CV2 (:246)
        return (int)d;
    }
    float f = (float)((double)v * p.gain[s]);                                   // FastISP stages the frame in float32 (isp_ops.py:178-187)
    f = fminf(fmaxf(f, 0.0f), 1.0f);
    return (int)__fmul_rn(f, 16383.0f);
}

__device__ __forceinline__ int isp_absdiff(int a, int b) { return a > b ? a - b : b - a; }

// v / 16383 as the reference forms it, then the colour matrix row by row in float64
__device__ __forceinline__ double isp_quot(int mode, int v) {
    return mode == YOND_ISP_SIDD ? (double)__fdiv_rn((float)v, 16383.0f) : (double)v / 16383.0;
}

__global__ __launch_bounds__(256) void render_srgb_kernel(const float* __restrict__ frame, const double* __restrict__ thr,
                                                          uint8_t* __restrict__ out_u8, float* __restrict__ out_f32, const IspParams p) {
    __shared__ __attribute__((aligned(16))) int s_q[ISP_LH * ISP_LW];
    __shared__ double s_t[257];                                                 // s_t[k] <= x < s_t[k + 1]  <=>  code k
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * ISP_TW, y0 = blockIdx.y * ISP_TH;
    const int H = p.H, W = p.W;
    if (out_u8) {
        for (int k = tid; k < 257; k += 256) s_t[k] = k == 0 ? 0.0 : (k == 256 ? __builtin_huge_val() : thr[k - 1]);
    }
    // stage: float4 groups of a row; a group inside the frame of a plain Bayer input is one 16-byte load (reversed for a left-right flip)
    const bool vec = p.layout == YOND_ISP_BAYER && (W & 3) == 0 && (((uintptr_t)frame) & 15) == 0;
    for (int it = tid; it < ISP_LH * (ISP_LW / 4); it += 256) {
        const int r = it / (ISP_LW / 4), g = it % (ISP_LW / 4);
        const int ly = y0 - 1 + r, lx = x0 - 4 + 4 * g;                         // logical (RGGB frame) coordinates, before the mirror
        int q[4] = {0, 0, 0, 0};
        if (ly <= H && lx + 3 >= -1 && lx <= W) {                               // (rows / groups beyond the halo are never read)
            const int y = isp_mirror(ly, H);
            const int sy = 2 * (y & 1);
            if (vec && lx >= 0 && lx + 3 < W) {
                const int ys = p.flip_ud ? H - 1 - y : y;
                const int xs = p.flip_lr ? W - 4 - lx : lx;
                const f32x4 v = *reinterpret_cast<const f32x4*>(frame + (size_t)ys * W + xs);
                if (p.flip_lr) { q[0] = isp_quant(p, v[3], sy); q[1] = isp_quant(p, v[2], sy + 1); q[2] = isp_quant(p, v[1], sy); q[3] = isp_quant(p, v[0], sy + 1); }
                else { q[0] = isp_quant(p, v[0], sy); q[1] = isp_quant(p, v[1], sy + 1); q[2] = isp_quant(p, v[2], sy); q[3] = isp_quant(p, v[3], sy + 1); }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (lx + j >= -1 && lx + j <= W) {
                        const int x = isp_mirror(lx + j, W);
                        q[j] = isp_quant(p, frame[isp_src(p, y, x)], sy + (x & 1));
                    }
                }
            }
        }
        *reinterpret_cast<int4*>(&s_q[r * ISP_LW + 4 * g]) = make_int4(q[0], q[1], q[2], q[3]);
    }
    __syncthreads();
    const int sx = tid & 31, sy = tid >> 5;
    const int x = x0 + 4 * sx, y = y0 + 2 * sy;                                 // the strip's first pixel: an R site
    if (x >= W || y >= H) return;
    int n[4][6];                                                                // rows y - 1 .. y + 2, columns x - 1 .. x + 4
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int* row = &s_q[(2 * sy + i) * ISP_LW + 4 * sx + 4];
        const int4 c = *reinterpret_cast<const int4*>(row);
        n[i][0] = row[-1]; n[i][1] = c.x; n[i][2] = c.y; n[i][3] = c.z; n[i][4] = c.w; n[i][5] = row[4];
    }
    int rgb[2][4][3];
#pragma unroll
    for (int i = 1; i <= 2; ++i) {
#pragma unroll
        for (int j = 1; j <= 4; ++j) {
            const int c = n[i][j], l = n[i][j - 1], r = n[i][j + 1], u = n[i - 1][j], d = n[i + 1][j];
            const int hor = (l + r + 1) >> 1, ver = (u + d + 1) >> 1;
            const bool row_r = i == 1, col_even = (j & 1) == 1;                 // compile-time after unrolling
            int R, G, B;
            if (row_r == col_even) {                                            // R or B site
                const int diag = (n[i - 1][j - 1] + n[i - 1][j + 1] + n[i + 1][j - 1] + n[i + 1][j + 1] + 2) >> 2;
                G = isp_absdiff(l, r) > isp_absdiff(u, d) ? ver : hor;          // ties go horizontal
                if (row_r) { R = c; B = diag; } else { B = c; R = diag; }
            } else {                                                            // G site: the row's colour left and right, the other above and below
                G = c;
                if (row_r) { R = hor; B = ver; } else { B = hor; R = ver; }
            }
            rgb[i - 1][j - 1][0] = R; rgb[i - 1][j - 1][1] = G; rgb[i - 1][j - 1][2] = B;
        }
    }
    const int ncol = min(4, W - x);                                             // 4, or 2 at the right edge of a frame with W % 4 == 2
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        uint32_t code[12];
        float val[12];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double d0 = isp_quot(p.mode, rgb[i][j][0]), d1 = isp_quot(p.mode, rgb[i][j][1]), d2 = isp_quot(p.mode, rgb[i][j][2]);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                double v = (d0 * p.m[3 * ch] + d1 * p.m[3 * ch + 1]) + d2 * p.m[3 * ch + 2];       // np.sum(images * ccms, -1)
                v = fmin(fmax(v, 0.0), 1.0);
                const int o = 3 * j + (p.order == YOND_ISP_BGR ? 2 - ch : ch);
                if (out_u8) {
                    int k = (int)(__builtin_amdgcn_exp2f(__builtin_amdgcn_logf(fmaxf((float)v, 1e-30f)) * (1.0f / 2.2f)) * 255.0f);
                    k = min(max(k, 0), 255);
                    while (k > 0 && s_t[k] > v) --k;                            // settle the float32 guess on the float64 table: exact
                    while (k < 255 && s_t[k + 1] <= v) ++k;
                    code[o] = (uint32_t)k;
                }
                if (out_f32) val[3 * j + ch] = (float)pow(v, p.inv_gamma);      // float form is RGB; pow in double, rounded once
            }
        }
        const size_t pix = (size_t)(y + i) * W + x;
        if (out_u8) {
            if (ncol == 4 && ((pix * 3) & 3) == 0) {                          // (a frame with W % 4 == 2 has odd rows off the 4-byte grid)
                IspRgb4 o;
#pragma unroll
                for (int w = 0; w < 3; ++w) o.w[w] = code[4 * w] | (code[4 * w + 1] << 8) | (code[4 * w + 2] << 16) | (code[4 * w + 3] << 24);
                *reinterpret_cast<IspRgb4*>(out_u8 + pix * 3) = o;
            } else {
#pragma unroll
                for (int e = 0; e < 12; ++e)
                    if (e < 3 * ncol) out_u8[pix * 3 + e] = (uint8_t)code[e];
            }
        }
        if (out_f32) {
#pragma unroll
            for (int e = 0; e < 12; ++e)
                if (e < 3 * ncol) out_f32[pix * 3 + e] = val[e];
        }
    }
}

extern "C" int yond_render_srgb(const float* frame, int H, int W, int flip_lr, int flip_ud, int layout, const double* gains,
                                const double* ccm, int mode, const double* thresholds, unsigned char* out_u8, int order,
                                float* out_f32, double gamma, void* stream) {
    if (!frame || !gains || !ccm || H < 2 || W < 2 || (H & 1) || (W & 1) || (!out_u8 && !out_f32)) return YOND_EINVAL;
    if (layout != YOND_ISP_BAYER && layout != YOND_ISP_PACKED4) return YOND_EINVAL;
    if (mode != YOND_ISP_SIDD && mode != YOND_ISP_FAST) return YOND_EINVAL;
    if (out_u8 && (!thresholds || (order != YOND_ISP_RGB && order != YOND_ISP_BGR) || (((uintptr_t)out_u8) & 3))) return YOND_EINVAL;
    if (out_f32 && !(gamma > 0.0)) return YOND_EINVAL;
    if (layout == YOND_ISP_PACKED4 && (flip_lr || flip_ud)) return YOND_EINVAL;
    IspParams p;
    for (int i = 0; i < 4; ++i) p.gain[i] = gains[i];
    for (int i = 0; i < 9; ++i) p.m[i] = ccm[i];
    p.inv_gamma = out_f32 ? 1.0 / gamma : 0.0;
    p.H = H; p.W = W; p.flip_lr = flip_lr != 0; p.flip_ud = flip_ud != 0; p.layout = layout; p.mode = mode; p.order = order;
    const dim3 grid((W + ISP_TW - 1) / ISP_TW, (H + ISP_TH - 1) / ISP_TH);
    if (grid.y > 65535) return YOND_EUNSUPPORTED;
    hipLaunchKernelGGL(render_srgb_kernel, grid, dim3(256), 0, (hipStream_t)stream, frame, thresholds, out_u8, out_f32, p);
    YOND_LAUNCH_CHECK();
    return YOND_OK;
}
