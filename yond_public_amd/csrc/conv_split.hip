// K2s dispatcher, weight packing and shape support of the split-operand kernel (conv_split_kernel.h); the kernel's
// instantiations live in conv_split_*.hip (one group per translation unit, compiled in parallel).
#include "conv_split_kernel.h"

SPLIT_VARIANTS(SPLIT_EXTERN)

// the channel-tile width the split kernel uses for a layer (0: not supported)
// ksize 1: the decoder's pixel-shuffle GEMM (cout = 4 sub-positions x channels of an output pixel; the descriptor has
// shuffle = 1): 48-channel steps, 64-wide tiles that must not straddle two sub-positions
extern "C" int yond_conv_split_supported(int ksize, int stride, int cin, int cout) {
    if (ksize == 1) {
        if (!(stride == 1 && cin > 0 && cin % 48 == 0 && cout > 0 && cout % 4 == 0)) return 0;
        return (cout / 4) % 64 == 0 ? 64 : ((cout / 4) % 32 == 0 ? 32 : 0);       // a tile may not straddle two sub-positions
    }
    if (ksize != 3 || (stride != 1 && stride != 2) || cin <= 0 || cout <= 0 || cin % 16 != 0 || cout % 32 != 0) return 0;
    if (stride == 2) return cout % 64 == 0 ? 64 : 0;
    return cout % 64 == 0 ? 64 : 32;
}

// OIHW fp32 weights -> the kernel's LDS image order [cout tile][cin chunk of 16][tap][channel half][part][tn][8 halves];
// parts = 2: h = fp16(w), l = fp16((w - h) * 2^11); parts = 1: h only.  dst: cout*cin*k*k * parts/2 floats.
// ksize 1 (w = the re-indexed [4*cout][cin][1][1] matrix of a transposed convolution): [cout tile][step of 48 channels]
// [chunk of 16][channel half][part][tn][8 halves].
extern "C" int yond_pack_conv_split_weight_f32(const float* w, int cout, int cin, int ksize, int tn, int parts, float* dst) {
    if (!w || !dst || (ksize != 3 && ksize != 1) || (tn != 32 && tn != 64 && !(tn == 128 && parts == 1)) || cout % tn != 0 || cin % 16 != 0 || (parts != 1 && parts != 2)) return YOND_EINVAL;
    _Float16* o = (_Float16*)dst;
    for (size_t i = 0, n = (size_t)cout * cin * ksize * ksize; i < n; ++i)
        if (!(fabsf(w[i]) <= 65504.0f)) return YOND_EUNSUPPORTED;          // its h half would be +-inf
    if (ksize == 1) {
        if (cin % 48 != 0) return YOND_EINVAL;
        for (int ct = 0; ct < cout / tn; ++ct)
            for (int ch = 0; ch < cin / 16; ++ch)              // (step, chunk) in order = chunk index
                for (int hh = 0; hh < 2; ++hh)
                    for (int p = 0; p < parts; ++p)
                        for (int j = 0; j < tn; ++j)
                            for (int e = 0; e < 8; ++e) {
                                const float v = w[(size_t)(ct * tn + j) * cin + ch * 16 + hh * 8 + e];
                                const _Float16 h = (_Float16)v;
                                *o++ = p == 0 ? h : (_Float16)((v - (float)h) * 2048.0f);
                            }
        return YOND_OK;
    }
    const int taps = 9;
    for (int ct = 0; ct < cout / tn; ++ct)
        for (int ch = 0; ch < cin / 16; ++ch)
            for (int tap = 0; tap < taps; ++tap)
                for (int hh = 0; hh < 2; ++hh)
                    for (int p = 0; p < parts; ++p)
                        for (int j = 0; j < tn; ++j)
                            for (int e = 0; e < 8; ++e) {
                                const int co = ct * tn + j, ci = ch * 16 + hh * 8 + e;
                                const float v = w[((size_t)co * cin + ci) * taps + tap];
                                const _Float16 h = (_Float16)v;
                                *o++ = p == 0 ? h : (_Float16)((v - (float)h) * 2048.0f);
                            }
    return YOND_OK;
}

// The same packing on the device (training: the weights change every step and never leave HBM).  One thread per 8 halves of the
// destination; a weight outside fp16's range sets bit 0 of *status (when given) instead of failing the call.
__global__ __launch_bounds__(256) void pack_split_weight_kernel(const float* __restrict__ w, int cout, int cin, int taps, int tn, int parts,
                                                                uint4* __restrict__ dst, size_t ngroups, int* __restrict__ status) {
    const size_t gi = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (gi >= ngroups) return;
    size_t g = gi;
    const int j = (int)(g % tn); g /= tn;
    const int p = (int)(g % parts); g /= parts;
    const int hh = (int)(g % 2); g /= 2;
    const int tap = (int)(g % taps); g /= taps;
    const int nch = cin / 16;
    const int ch = (int)(g % nch), ct = (int)(g / nch);
    const int co = ct * tn + j;
    union { _Float16 h[8]; uint4 v; } u;
    bool over = false;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int ci = ch * 16 + hh * 8 + e;
        const float v = w[((size_t)co * cin + ci) * taps + tap];
        over |= !(fabsf(v) <= 65504.0f);
        const _Float16 h = (_Float16)v;
        u.h[e] = p == 0 ? h : (_Float16)((v - (float)h) * 2048.0f);
    }
    dst[gi] = u.v;
    if (over && status) atomicOr(status, 1);
}

extern "C" int yond_pack_conv_split_weight_dev_f32(const float* w, int cout, int cin, int ksize, int tn, int parts, float* dst, int* status,
                                                   void* stream) {
    if (!w || !dst || (ksize != 3 && ksize != 1) || (tn != 32 && tn != 64 && !(tn == 128 && parts == 1)) || cout % tn != 0 || cin % 16 != 0 || (parts != 1 && parts != 2)) return YOND_EINVAL;
    if (ksize == 1 && cin % 48 != 0) return YOND_EINVAL;
    const int taps = ksize * ksize;
    const size_t ngroups = (size_t)cout * cin * taps * parts / 8;
    hipLaunchKernelGGL(pack_split_weight_kernel, dim3((unsigned)((ngroups + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, cout, cin, taps, tn,
                       parts, (uint4*)dst, ngroups, status);
    YOND_LAUNCH_CHECK();
    return YOND_OK;
}

// All of a training step's layers in ONE launch (45 launches of ~7 us before): desc[l] = {source offset (floats) in src, cout, cin,
// taps, tn, destination offset (floats) in dst, first 16-byte group of the layer}; a thread finds its layer by bisection.
__global__ __launch_bounds__(256) void pack_split_weight_batch_kernel(const float* __restrict__ src, const long long* __restrict__ desc, int nlayers,
                                                                      float* __restrict__ dst, size_t ngroups, int* __restrict__ status) {
    const size_t gi = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (gi >= ngroups) return;
    int lo = 0, hi = nlayers - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((size_t)desc[mid * 7 + 6] <= gi) lo = mid; else hi = mid - 1;
    }
    const long long* dl = desc + lo * 7;
    const float* w = src + dl[0];
    const int cin = (int)dl[2], taps = (int)dl[3], tn = (int)dl[4];
    size_t g = gi - (size_t)dl[6];
    const size_t gl = g;
    const int j = (int)(g % tn); g /= tn;
    const int p = (int)(g % 2); g /= 2;
    const int hh = (int)(g % 2); g /= 2;
    const int tap = (int)(g % taps); g /= taps;
    const int nch = cin / 16;
    const int ch = (int)(g % nch), ct = (int)(g / nch);
    const int co = ct * tn + j;
    union { _Float16 h[8]; uint4 v; } u;
    bool over = false;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int ci = ch * 16 + hh * 8 + e;
        const float v = w[((size_t)co * cin + ci) * taps + tap];
        over |= !(fabsf(v) <= 65504.0f);
        const _Float16 h = (_Float16)v;
        u.h[e] = p == 0 ? h : (_Float16)((v - (float)h) * 2048.0f);
    }
    ((uint4*)(dst + dl[5]))[gl] = u.v;
    if (over && status) atomicOr(status, 1);
}

extern "C" int yond_pack_conv_split_weights_batch_dev_f32(const float* src, const long long* desc, int nlayers, float* dst, size_t ngroups,
                                                          int* status, void* stream) {
    if (!src || !desc || !dst || nlayers <= 0 || ngroups == 0) return YOND_EINVAL;
    hipLaunchKernelGGL(pack_split_weight_batch_kernel, dim3((unsigned)((ngroups + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src, desc, nlayers,
                       dst, ngroups, status);
    YOND_LAUNCH_CHECK();
    return YOND_OK;
}

// ---- the dispatcher: CHOOSE a variant of the table (conv_split_kernel.h), then LAUNCH it.  Choosing is host arithmetic on the descriptor's numbers
// alone -- no pointer is dereferenced, no HIP call made -- so which instantiation a descriptor gets can be asked without a GPU
// (yond_conv_split_variant; tests/test_split_dispatch.py).  split_refuse says which descriptors are errors, the split_pick_* functions hold the
// heuristics: whatever reaches them has a variant.
namespace {

// what the descriptor says about the layer, worked out once
struct SplitLayer {
    int parts;                      // 2: split operands (algo 3), 1: h only (algo 4)
    int tn;                         // yond_conv_split_supported's tile width (the weights may be packed for 128 instead: half128*)
    // tensor formats (include/yond_hip.h): split planes in (LDS-DMA or register staging) / out (stored from the accumulator layout), planes
    // of 4 channels for the float32 tensors that are read as residuals
    // (parts 1 -- the fp16 path: the same formats with H-ONLY planes, [n][C/16][channel half][units]: 2 bytes per element)
    bool isp, osp, ip4, op4, rp4;
    bool half128, half128s2, half128k1;
};

// elements of a whole split-plane tensor (planes staged through registers are addressed with 32-bit element offsets)
long long sp_elems(int n, int c, int h, int w) { return (long long)n * (c / 16) * 4 * YOND_SP_PLANE_UNITS(h, w) * 4; }

// 12-row or 8-row tiles (64- and 128-channel kernels): 256 persistent workgroups walk the tiles in rounds, so a launch costs
// rounds x rows per tile; a row of a 12-row tile is ~10 % cheaper (0.59 instead of 0.78 KiB of LDS fragments per MFMA, 1.5x the MFMA
// work per barrier).  The full frames' levels (94 / 188 / 376 / 752 rows) fill whole rounds of 12-row tiles (1 / 2 / 4 / 8); batches of small
// images do not: 8- and 16-row images are padded 1.5x by 12-row tiles and are exact in 8-row tiles, 32-row images of a batch of 64
// take 1.5 rounds of 12-row tiles.  8-row tiles when they are >= 7 % cheaper by that count; fewer than 256 tiles: 8-row.
bool split_takes_12_rows(const YondConvDesc& d, int tn) {
    const long long t12 = split_tiles(d, 12, tn);
    const long long r12 = split_rounds(t12), r8 = split_rounds(split_tiles(d, 8, tn));
    return t12 >= 256 && !(8000 * r8 < 10044 * r12);              // cost8 = 8 r8 < 0.93 x cost12 = 0.93 x 10.8 r12
}

// Folded tiles (conv_split_kernel.h, FOLD), images at most 16 pixels wide -- the deepest levels of a batch of small blocks: a 32-pixel MFMA row
// would be half padding, so f = 2 / 4 sub-tiles of 16 / 8 columns (of one image or of several) share it.  th: rows of a sub-tile (the 3x3
// layers fold 4-row tiles, one row per wave; the decoder GEMM its 8-row tiles); 64-channel tiles throughout.  Every site has its own acceptance
// rule on the rounds and its own 32-bit bound (`fits`: a sub-tile of another image is addressed from sub-tile 0's base, at most f - 1 images further).
struct SplitFold { int f; long long rounds; };
SplitFold split_fold(const YondConvDesc& d, int th) {
    const int f = d.Wo <= 8 ? 4 : 2;
    return {f, split_rounds(split_fold_tiles(d, th, 64, f))};
}

// the h-only stride-2 layers: 8-row tiles (two output rows per wave) where they fill the persistent workgroups: the 4-row form's steps are bound by
// LDS reads (2.0 KiB of fragments per MFMA with h-only operands; conv_split_kernel.h, SPLIT_GROUP_H_S2_TALL).  engine.py (_conv, `ws2`) repeats
// this count for the 128-channel form, because it packs the weights before it has a descriptor: keep the two in step.
bool split_s2_h_tall(const YondConvDesc& d) { return split_tiles(d, 8, d.tn) >= 256 && yond_exp_long("YOND_SPLIT_S2_TALL", 1) != 0; }

// the decoder GEMM with two sub-positions per 64-wide tile (descriptor shuffle 2; conv_split_kernel.h, S2): Cr = Cout / 4 output channels,
// GEMM columns ordered [dy][channel block of 32][dx][32]; src1's K range = [Cr channels at dx = 0 | the same at dx = 1 |
// zero-weight channels up to a multiple of 48], split-plane inputs.  One form per operand kind: refusals only.
int split_choose_sub2(const YondConvDesc& d, SplitVariant* v) {
    const int Cr = d.Cout / 4;
    const int pad = d.C1 - 2 * Cr;
    if (d.ksize != 1 || d.stride != 1 || d.Cout % 128 || d.tn != 64 || d.C0 % 16 || pad < 0 || pad >= 48 || pad % 16 ||
        (d.C0 + d.C1) % 48 || d.in_fmt != YOND_FMT_SPLIT_PLANES || d.out_fmt == YOND_FMT_SPLIT_PLANES || d.res_fmt || d.pre_act || d.res ||
        d.out4_dst || d.post_act == 1 || d.Ho != d.H || d.Wo != d.W || !d.src1)
        return YOND_EUNSUPPORTED;
    if (sp_elems(d.N, d.C0, d.H, d.W) >= 0x7fffffffLL || sp_elems(d.N, Cr, 2 * d.H, 2 * d.W) >= 0x7fffffffLL) return YOND_EUNSUPPORTED;
    *v = d.algo == 3 ? SV_k1_8x64_split_reg_f32_sub2 : SV_k1_8x64_h_reg_f32_sub2;
    return YOND_OK;
}

// ---- refusals: YOND_OK, or the error of a descriptor no variant serves.  Sets L.
int split_refuse(const YondConvDesc& d, SplitLayer& L) {
    const int parts = L.parts = d.algo == 3 ? 2 : 1;
    const int tn = L.tn = yond_conv_split_supported(d.ksize, d.stride, d.C0 + d.C1, d.Cout);
    if (!tn || d.C0 % 16 != 0 || d.C1 % 16 != 0 || (d.shuffle != 0) != (d.ksize == 1)) return YOND_EUNSUPPORTED;
    // h-only operands (algo 4) may be packed for 128-channel tiles: 3x3 stride-1 layers with plain tensors (conv_split_kernel.h, HALF128)
    L.half128 = parts == 1 && d.tn == 128 && tn == 64 && d.ksize == 3 && d.stride == 1 && d.Cout % 128 == 0 && !d.out4_dst && !d.dst2 &&
                (d.out_fmt == YOND_FMT_SPLIT_PLANES || (!d.in_fmt && !d.out_fmt && !d.res_fmt));     // plain tensors, or a producer of the h-only flow
    // ... and the flow's stride-2 layers on 128-channel tiles (h-only planes in, planes of 4 channels out)
    L.half128s2 = parts == 1 && d.tn == 128 && tn == 64 && d.ksize == 3 && d.stride == 2 && d.Cout % 128 == 0 && d.in_fmt == YOND_FMT_SPLIT_PLANES &&
                  d.out_fmt == YOND_FMT_PLANES4;
    // ... and its decoder GEMMs whose output pixels have >= 128 channels (a 128-column tile may not straddle two sub-positions)
    L.half128k1 = parts == 1 && d.tn == 128 && tn == 64 && d.ksize == 1 && d.shuffle == 1 && (d.Cout / 4) % 128 == 0 && d.in_fmt == YOND_FMT_SPLIT_PLANES && !d.dst2;
    if (d.tn != tn && !L.half128 && !L.half128s2 && !L.half128k1) return YOND_EINVAL;             // the layout the weights were packed for
    if (d.post_act < 0 || d.post_act > 2) return YOND_EUNSUPPORTED;
    const bool isp = L.isp = d.in_fmt == YOND_FMT_SPLIT_PLANES, osp = L.osp = d.out_fmt == YOND_FMT_SPLIT_PLANES;
    const bool ip4 = L.ip4 = d.in_fmt == YOND_FMT_PLANES4, op4 = L.op4 = d.out_fmt == YOND_FMT_PLANES4, rp4 = L.rp4 = d.res_fmt == YOND_FMT_PLANES4;
    if (d.res_fmt != YOND_FMT_NHWC_F32 && !rp4) return YOND_EINVAL;
    if (isp && d.pre_act) return YOND_EUNSUPPORTED;             // the producer applied the activation
    // second output (SiLU in split planes): the stride-2 layers and the 64-column decoder GEMM with split-plane input and planes-of-4 output
    if (d.dst2 && !(isp && op4 && ((d.ksize == 3 && d.stride == 2 && d.Cout % 16 == 0) || (d.ksize == 1 && d.shuffle == 1 && tn == 64 && (d.Cout / 4) % 64 == 0)))) return YOND_EUNSUPPORTED;
    if (rp4 != (osp && d.res != nullptr)) return YOND_EUNSUPPORTED;   // a split-plane store reads its residual in planes of 4, nothing else does
    if (osp && d.res && !isp) return YOND_EUNSUPPORTED;              // ... and only conv2 of a block has one: split-plane input
    // 32-bit offsets: elements of a planes-of-4 tensor ...
    if (ip4 && (long long)d.N * (d.C0 > d.C1 ? d.C0 : d.C1) * d.H * d.W * (d.ksize == 1 ? 4 : 1) >= 0x7fffffffLL) return YOND_EUNSUPPORTED;
    // ... elements over the whole tensor where split planes are staged through registers (the decoder GEMM: the skip tensor at twice the resolution) ...
    if (isp && (d.ksize == 1 || d.stride == 2) &&
        (sp_elems(d.N, d.C0, d.H, d.W) >= 0x7fffffffLL || (d.ksize == 1 && sp_elems(d.N, d.C1, 2 * d.H, 2 * d.W) >= 0x7fffffffLL)))
        return YOND_EUNSUPPORTED;
    // ... unit offsets inside a plane and plane arithmetic
    if (isp && (long long)YOND_SP_PLANE_UNITS(d.H, d.W) * (d.ksize == 1 ? 4 : 1) * 16 * 4 >= 0x7fffffffLL) return YOND_EUNSUPPORTED;
    if (d.ksize == 1) {
        // the decoder GEMM: low-resolution input (C0) + skip tensor at the output resolution (C1), pixel-shuffle store
        if (d.pre_act || d.res || d.out4_dst || d.post_act == 1 || d.Ho != d.H || d.Wo != d.W || osp || ip4) return YOND_EUNSUPPORTED;
        // h-only operands: the decoder GEMM of the split-plane flow only (h-only planes in, planes of 4 channels out)
        if (parts == 1 && (!isp || !d.src1)) return YOND_EUNSUPPORTED;
        return YOND_OK;
    }
    if (d.stride == 2) {
        if (d.Ho != (d.H + 1) / 2 || d.Wo != (d.W + 1) / 2 || d.pre_act) return YOND_EINVAL;
        if (osp || ip4 || (op4 && d.res)) return YOND_EUNSUPPORTED;
        if (isp && parts == 1 && !op4) return YOND_EUNSUPPORTED;
        // 128-channel tiles: the 8-row form only (the caller packs 64-channel tiles for small images), and not with the second output (it spills: not built)
        if (L.half128s2 && (!split_s2_h_tall(d) || d.dst2)) return YOND_EUNSUPPORTED;
        return YOND_OK;
    }
    if (d.Ho != d.H || d.Wo != d.W) return YOND_EINVAL;
    // the fused output projection: 32 channels, split operands or the h-only flow's last convolution; never behind a split-plane store
    if (d.out4_dst && (tn != 32 || (parts != 2 && !isp) || osp)) return YOND_EUNSUPPORTED;
    if (op4) return YOND_EUNSUPPORTED;                          // (3x3 stride-1 layers store [N][H][W][C] or split planes)
    // the flow on h-only planes: conv1 (float32 planes of 4 in, SiLU staged, h-only store), conv2 / deep conv1 (h-only in by LDS-DMA), the last
    // convolution with the fused output projection -- nothing else
    if ((isp || osp) && parts == 1 && ((!isp && !d.pre_act) || (isp && !osp && !d.out4_dst))) return YOND_EUNSUPPORTED;
    return YOND_OK;
}

// ---- selection: the decoder GEMM
SplitVariant split_pick_k1(const YondConvDesc& d, const SplitLayer& L) {
    if (L.parts == 1) {
        if (L.half128k1) return SV_k1_8x128_h_reg_f32;
        if (d.dst2) return SV_k1_8x64_h_reg_f32_d2;
        // 64 columns: 16-row tiles (four rows per wave share every weight fragment: 1.25 instead of 1.5 KiB of LDS fragments per MFMA) where they fill the workgroups
        if (L.tn == 64 && L.op4 && split_tiles(d, 16, 64) >= 256 && yond_exp_long("YOND_SPLIT_K1_TALL", 1) != 0) return SV_k1_16x64_h_reg_f32;
        return L.tn == 32 ? SV_k1_8x32_h_reg_f32 : SV_k1_8x64_h_reg_f32;
    }
    if (L.isp && L.tn == 64 && d.Wo <= 16 && d.src1 && !d.dst2 && yond_exp_long("YOND_SPLIT_FOLD", 1) != 0) {
        // folded where that saves a round of 256 workgroups
        const SplitFold fo = split_fold(d, 8);
        const bool fits = (long long)d.H * d.W * (d.C0 > 4 * d.C1 ? d.C0 : 4 * d.C1) * 4 * fo.f < (1LL << 31);
        if (fits && fo.rounds < split_rounds(split_tiles(d, 8, 64))) return fo.f == 2 ? SV_k1_8x64_split_reg_f32_f2 : SV_k1_8x64_split_reg_f32_f4;
    }
    if (L.isp && d.dst2) return SV_k1_8x64_split_reg_f32_d2;
    if (L.isp) return L.tn == 32 ? SV_k1_8x32_split_reg_f32 : SV_k1_8x64_split_reg_f32;
    return L.tn == 32 ? SV_k1_8x32_split_f32_f32 : SV_k1_8x64_split_f32_f32;      // (32: level 1 -> 0, 32-channel output pixels)
}

// ---- selection: stride 2 (4 x 32 output pixels read 9 x 65 input pixels -- two weight buffers fit beside the two input images)
SplitVariant split_pick_s2(const YondConvDesc& d, const SplitLayer& L) {
    const bool fold_on = L.parts == 2 && d.Wo <= 16 && !d.src1 && !d.res && yond_exp_long("YOND_SPLIT_FOLD", 1) != 0;
    if (L.isp && fold_on) {
        // folded where that saves a round of 256 workgroups
        const SplitFold fo = split_fold(d, 4);
        const bool fits = (long long)d.H * d.W * d.C0 * 4 * fo.f < (1LL << 31);
        if (fits && fo.rounds < split_rounds(split_tiles(d, 4, 64))) {
            if (fo.f == 2) return d.dst2 ? SV_s2_4x64_split_reg_f32_d2_f2 : SV_s2_4x64_split_reg_f32_f2;
            return d.dst2 ? SV_s2_4x64_split_reg_f32_d2_f4 : SV_s2_4x64_split_reg_f32_f4;
        }
    }
    if (L.isp && L.parts == 1) {
        if (L.half128s2) return SV_s2_8x128_h_reg_f32;
        if (split_s2_h_tall(d)) return d.dst2 ? SV_s2_8x64_h_reg_f32_d2 : SV_s2_8x64_h_reg_f32;
        return d.dst2 ? SV_s2_4x64_h_reg_f32_d2 : SV_s2_4x64_h_reg_f32;
    }
    if (L.isp) return d.dst2 ? SV_s2_4x64_split_reg_f32_d2 : SV_s2_4x64_split_reg_f32;
    if (fold_on && !d.in_fmt && !d.out_fmt) {
        // the [N][H][W][C] form of the same (training's forward)
        const SplitFold fo = split_fold(d, 4);
        if (fo.rounds < split_rounds(split_tiles(d, 4, 64))) return fo.f == 2 ? SV_s2_4x64_split_f32_f32_f2 : SV_s2_4x64_split_f32_f32_f4;
    }
    return L.parts == 2 ? SV_s2_4x64_split_f32_f32 : SV_s2_4x64_h_f32_f32;
}

// ---- selection: 3x3 stride 1
SplitVariant split_pick_s1(const YondConvDesc& d, const SplitLayer& L) {
    const int parts = L.parts, tn = L.tn;
    const bool isp = L.isp, osp = L.osp, pre = d.pre_act != 0;
    const bool th12 = split_takes_12_rows(d, 64);
    // 32 -> 32 channels: two weight slices in all -- on two buffers they stay resident in LDS (conv_split_kernel.h, wres)
    const bool wres = parts == 2 && tn == 32 && d.Cout == 32 && d.C0 + d.C1 == 32 && yond_exp_long("YOND_SPLIT_WRES", 1) != 0;
    if (wres && isp && osp) return SV_s1_16x32_split_dma_sp_wres;
    if (wres && isp && d.out4_dst) return SV_s1_16x32_split_dma_f32_o4_wres;
    if (wres && osp && pre) return SV_s1_16x32_split_f32_sp_wres_pre;
    if ((isp || osp) && parts == 1) {
        // the flow on h-only planes
        if (!osp) return SV_s1_16x32_h_dma_f32_o4;
        if (L.half128) return isp ? SV_s1_8x128_h_dma_sp : SV_s1_8x128_h_f32_sp_pre;
        // four rows per wave where such tiles fill the workgroups (0.75 KiB of LDS fragments per MFMA instead of 0.89 / 1.17)
        // (32 channels: counted per channel tile)
        const bool t4_64 = tn == 64 && split_tiles(d, 16, 64) >= 256;
        const bool t4_32 = tn == 32 && split_tiles(d, 32, d.Cout) >= 256;
        if (isp) {
            if (t4_64) return SV_s1_16x64_h_dma_sp;
            if (t4_32) return SV_s1_32x32_h_dma_sp;
            if (tn == 64) return th12 ? SV_s1_12x64_h_dma_sp : SV_s1_8x64_h_dma_sp;
            return SV_s1_16x32_h_dma_sp;
        }
        if (t4_64) return SV_s1_16x64_h_f32_sp_pre;
        if (tn == 64) return th12 ? SV_s1_12x64_h_f32_sp_pre : SV_s1_8x64_h_f32_sp_pre;
        return SV_s1_16x32_h_f32_sp_pre;
    }
    if (isp || osp) {
        // Folded kernels: 4-row tiles, one row per wave (half the MFMAs per step and workgroup of the 8-row kernel: ~0.67x its step time, the
        // fragments of a single row are not shared between kernel rows); taken when the rounds of 256 workgroups say it is cheaper.
        int fold = 0;
        if (osp && (isp || pre) && tn == 64 && d.Wo <= 16 && !d.src1 && yond_exp_long("YOND_SPLIT_FOLD", 1) != 0) {
            const SplitFold fo = split_fold(d, 4);
            const bool fits = (long long)d.H * d.W * (d.C0 > d.Cout ? d.C0 : d.Cout) * 4 * fo.f < (1LL << 31);
            if (fits && 2 * fo.rounds < 3 * split_rounds(split_tiles(d, 8, 64))) fold = fo.f;
        }
        if (isp && osp) {
            if (fold) return fold == 2 ? SV_s1_4x64_split_dma_sp_f2 : SV_s1_4x64_split_dma_sp_f4;
            if (tn == 64) return th12 ? SV_s1_12x64_split_dma_sp : SV_s1_8x64_split_dma_sp;
            return SV_s1_16x32_split_dma_sp;
        }
        if (osp) {
            if (fold) return fold == 2 ? SV_s1_4x64_split_f32_sp_f2_pre : SV_s1_4x64_split_f32_sp_f4_pre;
            if (tn == 64 && th12) return pre ? SV_s1_12x64_split_f32_sp_pre : SV_s1_12x64_split_f32_sp;
            if (tn == 64) return pre ? SV_s1_8x64_split_f32_sp_pre : SV_s1_8x64_split_f32_sp;
            return pre ? SV_s1_16x32_split_f32_sp_pre : SV_s1_16x32_split_f32_sp;
        }
        if (tn == 64) return th12 ? SV_s1_12x64_split_dma_f32 : SV_s1_8x64_split_dma_f32;
        return d.out4_dst ? SV_s1_16x32_split_dma_f32_o4 : SV_s1_16x32_split_dma_f32;
    }
    // float32 tensors in and out
    if (L.half128) {
        if (split_takes_12_rows(d, 128)) return pre ? SV_s1_12x128_h_f32_f32_pre : SV_s1_12x128_h_f32_f32;
        return pre ? SV_s1_8x128_h_f32_f32_pre : SV_s1_8x128_h_f32_f32;
    }
    if (tn == 64) {
        if (parts == 2 && !pre && !d.src1 && !d.in_fmt && !d.out_fmt && !d.res_fmt && !d.out4_dst && !(d.ebatch && (d.escale || d.eshift)) && d.Wo <= 16 &&
            yond_exp_long("YOND_SPLIT_FOLD", 1) != 0) {
            // the plain [N][H][W][C] layer on images at most 16 pixels wide (training patches' deep levels): folded 4-row tiles, as in the split-plane flow above
            const SplitFold fo = split_fold(d, 4);
            const double cost_plain = th12 ? 1.35 * (double)split_rounds(split_tiles(d, 12, 64)) : (double)split_rounds(split_tiles(d, 8, 64));
            const bool fits = (long long)d.N * d.H * d.W * (d.C0 > d.Cout ? d.C0 : d.Cout) < (1LL << 31);
            if (fits && 0.667 * (double)fo.rounds < cost_plain) return fo.f == 2 ? SV_s1_4x64_split_f32_f32_f2 : SV_s1_4x64_split_f32_f32_f4;
        }
        if (parts == 2 && th12) return pre ? SV_s1_12x64_split_f32_f32_pre : SV_s1_12x64_split_f32_f32;
        if (parts == 2) return pre ? SV_s1_8x64_split_f32_f32_pre : SV_s1_8x64_split_f32_f32;
        if (th12) return pre ? SV_s1_12x64_h_f32_f32_pre : SV_s1_12x64_h_f32_f32;
        return pre ? SV_s1_8x64_h_f32_f32_pre : SV_s1_8x64_h_f32_f32;
    }
    if (parts == 2 && d.out4_dst)      // the last convolution of the network with the 1x1 output projection in its epilogue
        return pre ? SV_s1_16x32_split_f32_f32_o4_pre : SV_s1_16x32_split_f32_f32_o4;
    if (parts == 2) return pre ? SV_s1_16x32_split_f32_f32_pre : SV_s1_16x32_split_f32_f32;
    // h only, 32 channels: 32-row tiles where they fill the 256 persistent workgroups (counted per channel tile)
    if (split_tiles(d, 32, d.Cout) >= 256) return pre ? SV_s1_32x32_h_f32_f32_pre : SV_s1_32x32_h_f32_f32;
    return pre ? SV_s1_16x32_h_f32_f32_pre : SV_s1_16x32_h_f32_f32;
}

int split_choose(const YondConvDesc& d, SplitVariant* v) {
    if (d.shuffle == 2) return split_choose_sub2(d, v);
    SplitLayer L;
    const int rc = split_refuse(d, L);
    if (rc != YOND_OK) return rc;
    *v = d.ksize == 1 ? split_pick_k1(d, L) : (d.stride == 2 ? split_pick_s2(d, L) : split_pick_s1(d, L));
    return YOND_OK;
}

const char* const SPLIT_NAMES[SV_COUNT] = {SPLIT_VARIANTS(SPLIT_NAME)};

}  // namespace

int yond_conv_split_dispatch(const YondConvDesc& d, hipStream_t st) {
    SplitVariant v;
    const int rc = split_choose(d, &v);
    if (rc != YOND_OK) return rc;
    switch (v) {
        SPLIT_VARIANTS(SPLIT_LAUNCH_CASE)
        case SV_COUNT: break;
    }
    return YOND_EINVAL;
}

// the variant yond_conv2d_f32 launches for an algo 3 / 4 descriptor: its index in the table, or the (negative) error the launch would return
extern "C" int yond_conv_split_variant(const YondConvDesc* d) {
    if (!d || (d->algo != 3 && d->algo != 4) || d->N <= 0 || d->H <= 0 || d->W <= 0 || d->Ho <= 0 || d->Wo <= 0) return YOND_EINVAL;
    SplitVariant v;
    const int rc = split_choose(*d, &v);
    return rc != YOND_OK ? rc : (int)v;
}

extern "C" const char* yond_conv_split_variant_name(int variant) { return variant >= 0 && variant < SV_COUNT ? SPLIT_NAMES[variant] : nullptr; }
