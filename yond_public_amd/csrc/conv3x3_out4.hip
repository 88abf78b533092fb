// Last layer of a plain convolution stack (DnCNN, archs/comp.py:24-32): 3x3, stride 1, zero padding, Cin -> 4 channels,
//   dst = x + sign * (conv3x3(feat) + bias),
// fp32 operands, fp32-exact products (no operand is rounded to half: nothing here needs a range guard).
//
// Four output channels fill one eighth of a 32-row MFMA tile.  v_mfma_f32_4x4x1_16b_f32 has no such waste: its 16 blocks are 16
// independent 4 x 4 outer products, A = 4 output channels, B = 4 pixels, so ONE instruction is one (tap, input channel) k-step
// for 64 pixels and every product it forms is needed.  Lane l is pixel l (B operand: that pixel's feature at the channel) and
// supplies the weight of output channel l % 4 (A operand); register v of the result is output channel v of the lane's pixel.
//
// The B operand is the lane's OWN pixel for every tap: the kernel accumulates, per INPUT pixel and per tap column dx, the
// contributions T[dx] to the three output rows that read this input row, and moves the dx = 0 / 2 sums one lane right / left
// when an output row is complete:  out(y, x) = T0(y, x - 1) + T1(y, x) + T2(y, x + 1),  T_dx(y, x) = sum_dy sum_ci w[dy][dx][ci] f(y + dy - 1, x, ci).
// So a feature is read from HBM once (plus the halo: a wave covers 64 input columns for 62 output columns and walks a band of
// 2 * steps - 2 output rows downwards, two input rows per step; the host picks the step count, 4 .. 16, that balances the launch over the chip),
// passes through LDS once (the coalesced 16-byte loads hold 4 channels of 16 pixels per instruction; the MFMA wants one pixel per
// lane: a wave-private transpose, pixel stride KC + 4 floats, conflict-free for ds_read_b128), and the only repeated LDS reads
// are the weights (16 bytes per lane per 8 MFMAs).
//
// What bounds it: the matrix pipe.  The launch times fit 16 cycles per v_mfma_f32_4x4x1_16b_f32 on a SIMD (inferred from whole-launch
// times at two shapes, not measured on the instruction): half the rate of the 32x32x2 / 16x16x4 forms, which would need 8 or 4 times
// the output rows this layer has.  288 MFMAs per step of two input rows x 16 channels; two steps' global loads stay in flight.
//
// Non-finite containment: a value of input pixel (r, x) enters T(., x) of output rows r - 1 .. r + 1 only, and those enter
// output columns x - 1 .. x + 1: a NaN or infinity stays inside the 3x3 footprints that hold it.  Lanes and rows outside the
// image stage exact zeros.
#include "common.h"

namespace {

constexpr int O4_KC = 16;                 // input channels per step
constexpr int O4_MAX_STEPS = 16;          // steps of two input rows per band: a band is 2 * steps - 2 output rows (30 at 16 steps)
constexpr int O4_SEG = 62;                // output columns per wave (64 input columns)
constexpr int O4_PSTR = O4_KC + 4;        // LDS pixel stride in floats
constexpr int O4_MAX_CIN = 128;

struct O4Stage {
    f32x4 x[2];                           // the residual of the two output rows the step completes (lane = pixel)
    f32x4 g[2][4];                        // two input rows x 4 loads: 16 pixels x 4 channels x 4 lanes-per-pixel per instruction
};

__global__ __launch_bounds__(256, 2) void conv3x3_out4_kernel(const float* __restrict__ feat, int Cin, const float* __restrict__ wpk,
                                                              const float* __restrict__ bias, const float* __restrict__ x, float sign,
                                                              int H, int W, float* __restrict__ dst, int nseg, int nband, int steps, long long nitems) {
    __shared__ __attribute__((aligned(16))) float s_w[36 * O4_MAX_CIN];
    __shared__ __attribute__((aligned(16))) float s_f[4][2 * 64 * O4_PSTR];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < 9 * Cin; i += 256) *(f32x4*)(s_w + i * 4) = *(const f32x4*)(wpk + (size_t)i * 4);

    const long long item = (long long)blockIdx.x * 4 + wave;
    const bool live = item < nitems;
    const int seg = live ? (int)(item % nseg) : 0;
    const long long t = live ? item / nseg : 0;
    const int band = (int)(t % nband);
    const int n = (int)(t / nband);
    const int bh = 2 * steps - 2;                              // output rows per band
    const int y0 = band * bh, x0 = seg * O4_SEG - 1;           // first output row; input column of lane 0
    const int nch = Cin / O4_KC;
    const int total = steps * nch;
    const float* fimg = feat + (size_t)n * H * W * Cin;
    float* sf = s_f[wave];

    const int ox = x0 + lane;
    const bool has_x = x != nullptr;
    const float* xr = has_x ? x : feat;                        // (in bounds either way: a pixel of feat has at least 16 floats)
    // load role: instruction k of a row holds pixels 16 k .. 16 k + 15, lane -> (pixel lane / 4, channels 4 (lane % 4) ..)
    const int lp = lane >> 2, lq = lane & 3;
    // Straight-line code, every step, every lane: a conditional load would make the compiler wait for vmcnt(0) where the paths meet
    // and drain the stage in flight.  The residual rides in the stage (loads return in order: it is there when the features are), two
    // steps ahead of the rows' store; xr is x, or feat where there is none (never used then).
    auto load = [&](int it, O4Stage& st) {
        const int s = it / nch, c0 = (it % nch) * O4_KC;
#pragma unroll
        for (int j = 0; j < 2; ++j)
            st.x[j] = *(const f32x4*)(xr + (((size_t)n * H + min(max(y0 - 2 + 2 * s + j, 0), H - 1)) * W + min(max(ox, 0), W - 1)) * 4);
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
            const int gy = y0 - 1 + 2 * s + rr;
            const int cy = min(max(gy, 0), H - 1);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                // every lane loads (a branch per load would end in s_waitcnt vmcnt(0) and drain the stage in flight): outside the
                // image from the nearest pixel inside, replaced by zeros when it is staged (load_ok)
                const int gx = x0 + k * 16 + lp;
                const int cx = min(max(gx, 0), W - 1);
                st.g[rr][k] = *(const f32x4*)(fimg + ((size_t)cy * W + cx) * Cin + c0 + lq * 4);
            }
        }
    };

    f32x4 T[4][3];                        // output rows ra - 1 .. ra + 2 (ra = the step's first input row) x tap column
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int d = 0; d < 3; ++d) T[j][d] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const int co = lane & 3;
    const bool col_ok = live && lane >= 1 && lane <= O4_SEG && ox < W;
    f32x4 bv = {0.0f, 0.0f, 0.0f, 0.0f};
    if (bias) bv = *(const f32x4*)bias;

    // two steps' loads in flight behind the MFMAs (an HBM miss is longer than one step's 288 MFMAs): stages st0 / st1 alternate
    O4Stage st0, st1;
    load(0, st0);
    load(1, st1);                         // (total = steps * Cin / 16 is even: the host passes an even step count)
    __syncthreads();                      // the weights are in LDS: the only exchange between waves
    if (!live) return;
    // s_f[wave] is this wave's own: its LDS instructions execute in program order, so a transpose needs no barrier, only that the
    // compiler keeps the order (wavefront-scope fences: no instruction) -- the four waves drift apart and one's staging hides
    // under another's MFMAs
    auto wave_sync = [] {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    };
    auto step = [&](int it, O4Stage& st) {
        wave_sync();                      // the previous step's reads of s_f are issued
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
            const int gy = y0 - 1 + 2 * (it / nch) + rr;
            const bool row_ok = gy >= 0 && gy < H;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int gx = x0 + k * 16 + lp;
                const bool load_ok = row_ok && gx >= 0 && gx < W;
                const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
                *(f32x4*)(sf + (rr * 64 + k * 16 + lp) * O4_PSTR + lq * 4) = load_ok ? st.g[rr][k] : zero;
            }
        }
        wave_sync();
        f32x4 F[2][4];                    // compute role: lane = pixel, 16 channels of both rows
#pragma unroll
        for (int rr = 0; rr < 2; ++rr)
#pragma unroll
            for (int q = 0; q < 4; ++q) F[rr][q] = *(const f32x4*)(sf + (rr * 64 + lane) * O4_PSTR + q * 4);
        const int ra = y0 - 1 + 2 * (it / nch);
        const f32x4 xv[2] = {st.x[0], st.x[1]};
        load(min(it + 2, total - 1), st);                      // in flight behind this step's and the next one's MFMAs
        __builtin_amdgcn_sched_barrier(0);                     // (the scheduler would sink the loads to the end of the step)
        const int c = it % nch;
        const float* wc = s_w + ((size_t)c * 4 * 4 + co) * 4;  // [tap][Cin / 4][co][4]
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const f32x4 w4 = *(const f32x4*)(wc + ((size_t)(dy * 3 + dx) * (Cin / 4) + q) * 16);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        // input row ra feeds output row ra + 1 - dy (slot 2 - dy), row ra + 1 output row ra + 2 - dy (slot 3 - dy)
                        T[2 - dy][dx] = __builtin_amdgcn_mfma_f32_4x4x1f32(w4[e], F[0][q][e], T[2 - dy][dx], 0, 0, 0);
                        T[3 - dy][dx] = __builtin_amdgcn_mfma_f32_4x4x1f32(w4[e], F[1][q][e], T[3 - dy][dx], 0, 0, 0);
                    }
                }
        if (c == nch - 1) {
            // output rows ra - 1 and ra are complete
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int oy = ra - 1 + j;
                f32x4 o;
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const float left = __shfl_up(T[j][0][v], 1), right = __shfl_down(T[j][2][v], 1);
                    o[v] = ((left + T[j][1][v]) + right) + bv[v];
                }
                if (col_ok && oy >= y0 && oy < y0 + bh && oy < H) {
                    const size_t p = (((size_t)n * H + oy) * W + ox) * 4;
                    f32x4 r;
#pragma unroll
                    for (int v = 0; v < 4; ++v) r[v] = has_x ? xv[j][v] + sign * o[v] : sign * o[v];
                    *(f32x4*)(dst + p) = r;
                }
            }
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                T[0][d] = T[2][d];
                T[1][d] = T[3][d];
                T[2][d] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                T[3][d] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            }
        }
    };
    for (int it = 0; it < total; it += 2) {
        step(it, st0);
        step(it + 1, st1);
    }
}

}  // namespace

extern "C" int yond_pack_conv3x3_out4_weight_f32(const float* w, int cin, float* dst) {
    if (!w || !dst || cin <= 0) return YOND_EINVAL;
    if (cin % O4_KC != 0 || cin > O4_MAX_CIN) return YOND_EUNSUPPORTED;
    // [tap][cin / 4][co][cin % 4]: the 16 bytes a lane (output channel co) reads per tap and group of four input channels
    for (int tap = 0; tap < 9; ++tap)
        for (int ci = 0; ci < cin; ++ci)
            for (int co = 0; co < 4; ++co)
                dst[(((size_t)tap * (cin / 4) + ci / 4) * 4 + co) * 4 + ci % 4] = w[((size_t)co * cin + ci) * 9 + tap];
    return YOND_OK;
}

extern "C" int yond_conv3x3_out4_f32(const float* feat, int Cin, const float* wpk, const float* bias, const float* x, float sign,
                                     int N, int H, int W, float* dst, void* stream) {
    if (!feat || !wpk || !dst || N <= 0 || H <= 0 || W <= 0 || Cin <= 0) return YOND_EINVAL;
    if (sign != 1.0f && sign != -1.0f) return YOND_EINVAL;
    if (Cin % O4_KC != 0 || Cin > O4_MAX_CIN) return YOND_EUNSUPPORTED;
    // Band height.  The kernel is bound by the matrix pipe, which the waves of a SIMD share, and a workgroup puts one wave on each
    // SIMD of its CU: the launch takes about (steps per band) x (workgroups on the busiest of the 256 CUs).  The even step count
    // 4 .. 16 with the smallest product; among equals the tallest band (least halo: two extra input rows per band).
    const int nseg = (W + O4_SEG - 1) / O4_SEG;
    int steps = 0, nband = 0;
    long long nitems = 0, nblocks = 0, best = -1;
    for (int st = O4_MAX_STEPS; st >= 4; st -= 2) {
        const int nb = (H + 2 * st - 3) / (2 * st - 2);
        const long long blocks = ((long long)nseg * nb * N + 3) / 4;
        const long long cost = st * ((blocks + 255) / 256);
        if (best < 0 || cost < best) {
            best = cost;
            steps = st;
            nband = nb;
            nitems = (long long)nseg * nb * N;
            nblocks = blocks;
        }
    }
    if (nblocks > 0x7fffffffLL) return YOND_EUNSUPPORTED;
    hipLaunchKernelGGL(conv3x3_out4_kernel, dim3((unsigned)nblocks), dim3(256), 0, (hipStream_t)stream, feat, Cin, wpk, bias, x, sign,
                       H, W, dst, nseg, nband, steps, nitems);
    YOND_LAUNCH_CHECK();
    return YOND_OK;
}
