/* yond_hip.h -- C ABI of libyond_hip.so: the MI355X (gfx950) kernels behind YOND's per-image hot path.
 *
 * The reference (fenghansen/YOND_public) has no FFI: its hot path is Python over NumPy / cv2 / SciPy /
 * torch.nn.  The boundary a maintainer binds is therefore this C ABI, called through ctypes from the
 * Python functions that keep the reference's names.  Every entry point
 *   - takes plain device pointers (from torch.Tensor.data_ptr()), sizes and a hipStream_t (as void*),
 *   - is asynchronous on that stream, allocates nothing, keeps no state and owns none of its arguments,
 *   - returns 0 on success, a negative YOND_E* code for a rejected argument (nothing launched) or the
 *     positive hipError_t of a failed launch.
 * All images are float32.  "packed" means the 4-channel half-resolution view of a Bayer frame,
 * channel = 2*dy+dx  (utils/isp_ops.py:57-63).  Each function cites the reference lines it replaces
 * (paths relative to the reference root).
 */
#ifndef YOND_HIP_H
#define YOND_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define YOND_OK 0
#define YOND_EINVAL (-1)      /* bad pointer / size / flag */
#define YOND_EUNSUPPORTED (-2) /* valid request the kernels do not cover (e.g. channel count) */

/* Library / device probe.  Returns the ABI version (this header: YOND_ABI_VERSION; the loader refuses a mismatch). */
#define YOND_ABI_VERSION 8
int yond_abi_version(void);

/* ------------------------------------------------------------------------------------------------
 * K1  pack + VST + bias + normalise + reflect-pad + clamp            (memory bound, 8 B / Bayer px)
 * Replaces YOND_SIDD.py:251-269 (pack, *scale, bias LUT, VST, normalise), :281-282 (reflect pad to a
 * multiple of 32), :286 (clamp to [0,1]), utils/isp_algos.py:5-14 (VST) and the per-pixel evaluation
 * of the interp1d object returned by utils/isp_algos.py:128.  Also produces the per-image maximum that
 * archs/modules.py:15-21 (data_normalize) needs.
 *   bayer      [H][W]                      input frame (device)
 *   out        [Hp][Wp][4]                 Hp = h+pad_t+pad_b, Wp = w+pad_l+pad_r, h=H/2, w=W/2
 *   mode       0: identity (Simple_Denoiser, YOND_SIDD.py:238-243: pack, pad, clamp only)
 *              1: u = (VST(x*scale) - bias(max(x*scale,0)) - lo) / (hi - lo)
 *   lut_x/lut_y  knots of the bias LUT (float64 abscissae, float32 ordinates, device); lut_n = 0
 *              disables the bias correction (bias_corr=None).
 *   img_max    optional device float[1]: max over the clamped output (must be zeroed by the caller
 *              -- the function issues the memset itself on `stream`).
 * Arithmetic: float32 x*scale, then float64 in NumPy's staging with three shortcuts that stay below 1e-12 relative --
 * sqrt as a float32 estimate + one float64 Newton step, the LUT as per-interval coefficients a + b x, (v - lo) times the
 * reciprocal span -- and ONE rounding to float32: the result differs from the staged float64 evaluation by at most one
 * float32 ulp, and only where that evaluation lies within 1e-12 of a rounding boundary.  One exception, from the LUT's interval
 * lookup (one multiply on evenly spaced runs of knots, csrc/lut_table.h): a pixel within 1e-3 of a step of a knot may be evaluated
 * on the neighbouring interval, which moves the float64 value by at most |slope_next - slope_prev| * |x - knot| / (hi - lo)
 * (< 1e-9 on get_bias' tables).  tests/vst_model.py restates the evaluation and the bound; tests/test_hip_vst_edges.py asserts it
 * per element for every K1 entry point.
 * NaN / Inf pixels: the clamp is fminf(fmaxf(u, 0), 1), which returns the other operand for a NaN -- a NaN pixel gives 0 in every
 * mode and through every K1 entry point (torch.clamp would hand the NaN on to the network), and img_max ignores it; -inf gives 0;
 * +inf gives 1 without a bias LUT (with one it lies beyond the last knot, where the 1-D LUT has no value). */
int yond_pack_vst_norm_f32(const float* bayer, int H, int W, float* out, int pad_l, int pad_r, int pad_t,
                           int pad_b, int mode, double scale, double gain, double sigma, double lo,
                           double hi, const double* lut_x, const float* lut_y, int lut_n, float* img_max,
                           void* stream);

/* K1 with the 2-D bias LUT (YOND_SIDD.py:258-259 -> utils/isp_algos.py:162-231 BiasLUT.get_lut): lut_x = the table's x
 * knots in DN (x_lut * gain, float64), lut_y = the table row merged for sigma / gain (float64; the host interpolates the
 * two neighbouring sigma rows, :188-194).  Beyond the last knot: the last ordinate for one more interval, then
 * get_bias_points' closed form (:226-230).  Otherwise as yond_pack_vst_norm_f32 with mode 1. */
int yond_pack_vst_norm_biaslut_f32(const float* bayer, int H, int W, float* out, int pad_l, int pad_r, int pad_t,
                                   int pad_b, double scale, double gain, double sigma, double lo, double hi,
                                   const double* lut_x, const double* lut_y, int lut_n, float* img_max, void* stream);

/* The bias LUT alone on a flat float32 array (the callable get_bias returns, utils/isp_algos.py:128, or
 * BiasLUT.get_lut(x), :196-231): y_is_f64 selects float64 ordinates, biaslut the 2-D LUT's behaviour beyond the knots.
 * out: float64[n]. */
int yond_bias_eval_f32(const float* x, size_t n, const double* lut_x, const void* lut_y, int lut_n, int y_is_f64, int biaslut,
                       double gain, double sigma, double* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K4  clamp + crop + de-normalise + inverse VST + unpack (+ /scale, clip)          (8 B / Bayer px)
 * Replaces YOND_SIDD.py:286 (output clamp), :289-299 and utils/isp_algos.py:17-33 (inverse_VST).
 *   net_out  [Hp][Wp][4];  bayer_out [2h][2w];  crop origin (pad_t, pad_l)
 *   mode 0: identity (Simple_Denoiser :244-248), 1: algebraic inverse, 2: closed-form exact inverse
 *   clip01: apply the caller's .clip(0,1) (YOND_SIDD.py:389,407).
 * One rounding to float32 of the float64 evaluation; mode 2 maps z <= 0 to 0 as the reference's masked assignment does.
 * NaN / Inf inputs: the input clamp fminf(fmaxf(y, 0), 1) takes a NaN (and -inf) as 0 and +inf as 1 -- the output is finite for any input
 * (torch.clamp would keep the NaN). */
int yond_denorm_ivst_unpack_f32(const float* net_out, int Hp, int Wp, int pad_t, int pad_l, int h, int w,
                                float* bayer_out, int mode, double scale, double gain, double sigma,
                                double lo, double hi, int clip01, void* stream);

/* K1 / K4 for B equally sized frames that share every constant and the bias LUT -- the 32 blocks of a SIDD image, which the
 * reference sends through VST_Denoiser one by one with the same p and bias_func (YOND_SIDD.py:392-407): ONE launch each.
 *   bayer [B][H][W] -> out [B][Hp][Wp][4], img_max [B];   net_out [B][Hp][Wp][4] -> bayer_out [B][2h][2w].
 *   biaslut != 0: lut_y is float64, the merged row of the 2-D table (as yond_pack_vst_norm_biaslut_f32). */
int yond_pack_vst_norm_batch_f32(const float* bayer, int B, int H, int W, float* out, int pad_l, int pad_r, int pad_t, int pad_b,
                                 double scale, double gain, double sigma, double lo, double hi, const double* lut_x,
                                 const void* lut_y, int lut_n, int biaslut, float* img_max, void* stream);
int yond_denorm_ivst_unpack_batch_f32(const float* net_out, int B, int Hp, int Wp, int pad_t, int pad_l, int h, int w,
                                      float* bayer_out, int mode, double scale, double gain, double sigma,
                                      double lo, double hi, int clip01, void* stream);

/* Stand-alone elementwise VST / inverse VST on flat arrays (utils/isp_algos.py:5-14, 17-33) for the function
 * seam; the hot path uses the fused K1 / K4 above.  float32 -> float64 and float64 -> float64 as NumPy stages
 * them with np.float64 noise parameters. */
int yond_vst_elem_f32(const float* x, size_t n, double sigma, double mu, double gain, double* out, void* stream);
int yond_ivst_elem_f64(const double* z, size_t n, double sigma, double gain, int exact, double* out, void* stream);

/* Bayer <-> packed planar/NHWC4 copies (utils/isp_ops.py:57-63), bit exact. */
int yond_bayer2rggb_f32(const float* bayer, int H, int W, float* rggb /*[H/2][W/2][4]*/, void* stream);
int yond_rggb2bayer_f32(const float* rggb, int h, int w, float* bayer /*[2h][2w]*/, void* stream);

/* np.rot90(x, k, axes=(-2, -1)) on a stack [N][H][W] -> [N][H'][W'] (rot_bayer: utils/sidd_utils.py:198-213, used around
 * the denoiser when the runfile sets rot_cfa, YOND_SIDD.py:402-404, 462-464), bit exact. */
int yond_rot90_f32(const float* src, int N, int H, int W, int k, float* dst, void* stream);

/* Layout helpers for the archs plugin surface (NCHW tensors in, NCHW out; C == 4). */
int yond_nchw4_to_nhwc4_f32(const float* src, float* dst, int N, int H, int W, void* stream);
int yond_nhwc4_to_nchw4_f32(const float* src, float* dst, int N, int H, int W, void* stream);

/* Per-image maximum (archs/modules.py:18-19).  x: [N][elems]; partial: workspace float[N*256];
 * out: float[N].  Two launches, deterministic.  A NaN is DROPPED, not propagated (every step is fmaxf, which returns its other
 * operand): out[n] is the maximum of the image's non-NaN elements, -inf for an image that is all NaN -- where torch's x.max() returns
 * NaN.  A caller that needs to notice a NaN has to look for it itself; -inf and +inf are ordinary values here. */
int yond_image_max_f32(const float* x, int N, size_t elems, float* partial, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K2  convolutions of the denoiser as MFMA implicit GEMMs on NHWC float32 activations with float32 results.  `algo`
 * selects the arithmetic: 3 / 5 (the default path of engine.py) fp32-accurate split-operand products on the fp16 matrix
 * cores (v_mfma_f32_32x32x16_f16 / 32x32x8_f16, three per fp32 product block), 0 / 1 the fp32-input MFMA
 * (v_mfma_f32_32x32x2_f32 direct, v_mfma_f32_16x16x4_f32 Winograd), 2 / 4 fp16 operands (BASELINE cfg 5).
 * One descriptor covers: 3x3 stride 1 / stride 2 and 1x1 convolutions,
 * an input that is the channel concatenation of two tensors (torch.cat([up, skip], 1) is never
 * materialised), 2x2 stride-2 transposed convolution (as a 1x1 GEMM with a pixel-shuffle store), an
 * optional SiLU on the staged input, and the epilogue  v = acc*escale + eshift ; act(v) ; v += res.
 * Replaces nn.Conv2d / nn.ConvTranspose2d / SiLU / FiLM / residual at archs/modules.py:117-125,
 * 186-196, 221-233 and archs/Unet.py:55-104, 332-378, 424-470.
 * Weights must be packed by yond_pack_conv_weight_f32 (host side) for the same (taps, TN, KC). */
typedef struct YondConvDesc {
    const float* src0;    /* [N][H][W][C0] */
    const float* src1;    /* [N][H][W][C1] or NULL; with shuffle: the skip tensor at the OUTPUT resolution [N][2H][2W][C1],
                             read at the sub-position each channel block stores to (fused convT + cat + 1x1 shortcut) */
    int C0, C1;           /* Cin = C0 + C1; each a multiple of kc */
    int N, H, W;          /* input extent */
    int Ho, Wo;           /* GEMM-M extent: H/stride, W/stride (convT: H, W) */
    int Cout;             /* GEMM-N extent (convT: 4 * real Cout), multiple of 32 */
    int ksize;            /* 1 or 3 */
    int stride;           /* 1 or 2 (2 only with ksize 3) */
    int shuffle;          /* 1: convT 2x2 s2 store, dst is [N][2Ho][2Wo][Cout/4], GEMM column = sub-position * Cout/4 + channel;
                             2 (algo 3, split-plane inputs, Cout/4 = Cr a multiple of 32): the same with TWO sub-positions (dy, 0),
                             (dy, 1) per 64-wide channel tile -- GEMM columns ordered [dy][channel block of 32][dx][32]; the K range
                             of src1 is [Cr channels read at dx = 0 | the same channels read at dx = 1 | zero-weight channels up to
                             (C0 + C1) % 48 == 0], and the weight rows of a sub-position are zero in the other one's range:
                             src0 is staged once for both */
    int pre_act;          /* 0 none, 1 SiLU applied to the staged input */
    int post_act;         /* 0 none, 1 SiLU (algo 3 / 4, 3x3 only: the stored tensor is the consumer's SiLU input), 2 LeakyReLU(slope) */
    float slope;
    const float* wpk;     /* packed weights */
    const float* escale;  /* [ebatch ? N : 1][Cout'] or NULL (=1) ; Cout' = real Cout */
    const float* eshift;  /* [ebatch ? N : 1][Cout'] or NULL (=0) */
    int ebatch;
    const float* res;     /* residual, same shape as dst, or NULL */
    float* dst;           /* [N][Ho][Wo][Cout]  (shuffle: see above) */
    int tn;               /* channel-tile width the weights were packed for (32 or 64, from yond_conv_config) */
    int kc;               /* channel chunk the weights were packed for (8 or 16, from yond_conv_config; 0 = default) */
    int algo;             /* 0 direct implicit GEMM, fp32 MFMA; 1 Winograd F(2x2,3x3), fp32 MFMA (3x3 stride 1 only; wpk from
                             yond_pack_conv_wino_weight_f32, tn = 64, see yond_conv_wino_supported); 2 direct implicit GEMM
                             on the fp16 MFMA (operands rounded to half at the matrix core, fp32 accumulate, fp32 tensors:
                             BASELINE cfg 5; same packed weights as algo 0); 3 direct implicit GEMM on the fp16 MFMA with
                             fp32-accurate SPLIT operands (a = h + l 2^-11, three fp16 products per fp32 product, fp32
                             accumulate; 3x3 only, wpk from yond_pack_conv_split_weight_f32 with parts = 2, tn from
                             yond_conv_split_supported); 4 the same kernel with h only = plain fp16 MFMA (parts = 1); 5 the split-operand
                             arithmetic of algo 3 in the generic kernel of algo 0 for the 1x1 / transposed layers (wpk from
                             yond_pack_conv_weight_split_f32, tn / kc from yond_conv_config); 6 the decoder GEMM of algo 3 (ksize 1, split
                             planes in; shuffle 1 with planes of 4 out, or shuffle 2 at 32-channel output pixels with [N][H][W][C] out;
                             the same packed weights, the same bits) with the channel
                             tile's weights stationary in LDS and the pixels loaded straight into registers -- only for a descriptor
                             yond_gemm_k1_stationary_supported accepts, YOND_EUNSUPPORTED otherwise; 7 the 3x3 stride-2 layer of algo 3
                             (split planes in, planes of 4 out, with or without dst2; the same packed weights, the same bits) on 8-row
                             tiles, two output rows per wave, one or two input images in LDS (csrc/conv_s2_tall.hip) -- only for a descriptor
                             yond_conv_s2_tall_supported accepts, YOND_EUNSUPPORTED otherwise */
    /* Fused output projection (archs/Unet.py:466-470 `conv10` + residual + data_inv_normalize, i.e. what yond_conv_out_f32
       does as a kernel of its own): when out4_dst is set the convolution must produce ONE 32-channel tile (Cout = tn = 32,
       algo 3, stride 1); its result v is not stored (dst may be NULL) and out4_dst[n][y][x][c] =
       ((sum_k out4_w[c][k] v[k]) + out4_b[c] + out4_x / ub) * ub is written instead (same operation order as
       yond_conv_out_f32: bit-identical). */
    const float* out4_w;  /* [4][Cout] */
    const float* out4_b;  /* [4] or NULL */
    const float* out4_x;  /* NHWC4 network input [N][Ho][Wo][4] (global residual) or NULL */
    const float* out4_ub; /* [N] per-image maximum (data_normalize) or NULL */
    float* out4_dst;      /* [N][Ho][Wo][4] or NULL (no fused projection) */
    /* Range guard of the half-precision operand paths (algo 2..5): a device word (or NULL) into which a kernel ORs
       YOND_STATUS_HALF_OVERFLOW when a staged activation does not fit fp16 (|a| > 65504: its h half would be +-inf and the
       result silently wrong).  The caller zeroes it, reads it after the forward and falls back to the fp32-input MFMA
       kernels (algo 0 / 1).  Weights are checked by the packing functions (YOND_EUNSUPPORTED). */
    unsigned int* status;
    /* Tensor formats (algo 3 and 4 only; 0 = [N][H][W][C] float32, the default everywhere).
       1 = SPLIT PLANES: what the consumer's LDS staging holds, stored once by the producer -- every value a (after the
       consumer's pre-activation, which the PRODUCER applies: post_act) as the half pair h = fp16(a), l = fp16((a - h) 2^11),
       laid out [N][C/16][channel half 0..1][part h, l][YOND_SP_PLANE_UNITS(H, W)] in units of 16 bytes = 8 consecutive
       channels of one pixel, pixel index y*W + x; the units behind H*W of every plane are a zero pad that the CALLER
       zeroes once (producers never write it; consumers read conv zero padding from it).  A consumer (in_fmt 1: src0 and
       src1, pre_act must be 0) stages its input by LDS-DMA alone; a producer (out_fmt 1: dst, 3x3 stride 1, no res,
       no fused projection) stores from the accumulator layout without an LDS transpose.  Bit-identical to staging the
       float32 tensor (the same split of the same float32 value).
       With algo 4 (h-only operands: the fp16 path, BASELINE cfg 5) format 1 means H-ONLY PLANES: the h halves alone,
       [N][C/16][channel half 0..1][YOND_SP_PLANE_UNITS(H, W)] units -- 2 bytes per element, the value every algo-4 consumer would have
       rounded to when staging the float32 tensor; the same roles (3x3 stride-1 producers / consumers, the stride-2 layers, the decoder
       GEMM with shuffle 1 or 2, dst2, the fused projection with split-plane input), the same zero pad, the same residual rule. */
    int in_fmt, out_fmt;
    /* 2 = PLANES OF 4 CHANNELS, float32 [N][C/4][H*W][4]: the format of the tensors that are read as RESIDUALS by a
       split-plane store (res_fmt 2 is required with out_fmt 1 and a residual, and only there): in the accumulator layout
       a lane reads / writes 16 bytes of its own pixel and a wave 512 contiguous bytes.  Producers: the stride-2 and
       transposed layers (out_fmt 2), yond_conv_in_f32; consumers: the register-staged input of a 3x3 layer (in_fmt 2:
       src0 and src1) and `res`. */
    int res_fmt;
    /* Measurement aid (algo 3 / 4; NULL = off): workgroup 0 adds its elapsed shader cycles (s_memtime) to clk[0] and the
       elapsed 100 MHz reference ticks (s_memrealtime) to clk[1]: over many launches clk[0] / clk[1] * 100 MHz is the clock the
       chip really held inside these kernels (bench.py `gfx_clock.in_kernel_mhz`).  Two counter reads and two atomics per launch. */
    unsigned long long* clk;
    /* Order in which the persistent workgroups of algo 3 / 4 walk the pixel tiles: 0 first row of tiles to last, 1 last to
       first.  A chain of memory-bound layers alternates it: the consumer then starts with the rows its producer wrote (and read)
       LAST, which are still in the 256 MB Infinity Cache, instead of the rows that were evicted first.  Results do not depend on it. */
    int tile_order;
    /* Second output of a stride-2 layer (algo 3 at split precision, split-plane input, out_fmt 2; NULL = none): SiLU of the
       stored value in SPLIT PLANES -- the tensor the next residual block's conv1 would otherwise build in its own staging
       (SiLU + split of every input pixel, once per output-channel tile: 4 / 8 times at 256 / 512 channels); with it that conv1
       stages by LDS-DMA alone (in_fmt 1, pre_act 0).  Same bits as the consumer-side staging.  Zero pad as for every
       split-plane tensor. */
    float* dst2;
} YondConvDesc;
#define YOND_STATUS_HALF_OVERFLOW 1u
#define YOND_FMT_NHWC_F32 0
#define YOND_FMT_SPLIT_PLANES 1
#define YOND_FMT_PLANES4 2
/* 16-byte units per plane of a split-plane tensor: H*W pixels + at least one zero unit, rounded to 128 bytes */
#define YOND_SP_PLANE_UNITS(H, W) ((((H) * (W)) + 8) / 8 * 8)
/* bytes of a split-plane tensor of C channels (C a multiple of 16); of an h-only tensor (algo 4): half of it */
#define YOND_SP_BYTES(N, C, H, W) ((size_t)(N) * ((C) / 16) * 4 * (size_t)YOND_SP_PLANE_UNITS(H, W) * 16)
#define YOND_HP_BYTES(N, C, H, W) ((size_t)(N) * ((C) / 16) * 2 * (size_t)YOND_SP_PLANE_UNITS(H, W) * 16)

/* Tile configuration for a convolution (needed to pack weights): kc = channel chunk, tn = channel-tile width.
 * N, Ho, Wo (GEMM-M extent; 0 = unknown) let the library pick the tn that fills its persistent grid best. */
int yond_conv_config(int ksize, int stride, int cin, int cout, int shuffle, int N, int Ho, int Wo, int* tn, int* kc);
/* Host-side weight packing: w is OIHW [cout][cin][k][k] (Conv2d) -- for a transposed conv pass the
 * already re-indexed [4*cout][cin][1][1] matrix.  dst has cout*cin*k*k floats. */
int yond_pack_conv_weight_f32(const float* w, int cout, int cin, int ksize, int tn, int kc, float* dst);
/* as yond_pack_conv_weight_f32, every weight stored as the half pair {fp16(w), fp16((w - fp16(w)) * 2^11)} (algo 5) */
int yond_pack_conv_weight_split_f32(const float* w, int cout, int cin, int ksize, int tn, int kc, float* dst);
/* Non-finite inputs (algo 0 and 1, the fp32-input MFMA kernels): an output is finite, and as accurate as without them, whenever its input FOOTPRINT
 * holds no NaN or infinity -- the ksize x ksize window for algo 0; for algo 1 the 4 x 4 input tile of the output's 2 x 2 patch (rows 2i - 1 .. 2i + 2,
 * columns 2j - 1 .. 2j + 2 for outputs (2i .. 2i + 1, 2j .. 2j + 1)) is what is promised.  (By the zeros of B^T an output of F(2x2, 3x3) reads only
 * planes fed by its own 3 x 3 window, and the kernel was measured to confine a NaN / infinity to exactly that window; the tile is the rule that survives
 * another transform.)  Nothing else leaks: lanes outside the image read pixel 0 of the source (element 0 of the residual) and discard it, so a NaN there
 * stays in its own footprint (tests/test_hip_fp32_mfma.py).  Accuracy of algo 1 inside the window: every input is multiplied by sums of ALL three taps of
 * its filter row and column (U = G g G^T) that cancel only algebraically, so an output's rounding error scales with |input| x the largest tap it meets,
 * not with the products it keeps (tests/fp32_model.py has the per-output bound, DESIGN section 3 the measured ratio to a direct convolution). */
int yond_conv2d_f32(const YondConvDesc* desc, void* stream);

/* Winograd F(2x2,3x3) variant of the 3x3 stride-1 convolution (same descriptor, algo = 1): 16 instead of 36
 * multiplications per output patch, fp32 throughout; the result differs from the direct kernel by rounding order
 * only.  yond_conv_wino_supported: the channel-tile width the kernel would use for (cin, cout) -- 64
 * (cout % 64 == 0: 8 x 32 pixel tiles), 32 (cout % 32 == 0: 16 x 32 pixel tiles) or 0 (not supported; cin % 8 != 0); put it in desc.tn and pass it to the packing function.
 * Weights: w OIHW [cout][cin][3][3] -> dst, 16*cout*cin floats (U = G g G^T in float64, rounded once). */
int yond_conv_wino_supported(int cin, int cout);
int yond_pack_conv_wino_weight_f32(const float* w, int cout, int cin, int tn, float* dst);

/* Split-operand fp16-MFMA form of the 3x3 convolutions (same descriptor, algo = 3 or 4; archs/modules.py:117-125,
 * 163-233 are the layers it serves).  Each fp32 operand is split when it is staged into LDS: h = fp16(a),
 * l = fp16((a - h) * 2^11); a*w = h_a h_w + 2^-11 (h_a l_w + l_a h_w) on v_mfma_f32_32x32x16_f16 with fp32
 * accumulation -- 22-23 significant bits per operand, error vs a float64 convolution no larger than the fp32 kernels'.
 * Precondition: |activations|, |weights| <= 65504 -- enforced: the packing functions return YOND_EUNSUPPORTED for a weight
 * outside that range and the kernels report an activation outside it through YondConvDesc.status.  yond_conv_split_supported: channel-tile width (64, 32) or 0; h-only weights (parts = 1) of a 3x3 stride-1 layer whose output channels divide by 128 may also be packed for tn = 128 (YondConvDesc.tn = 128, algo 4, plain tensors).
 * Weights: w OIHW [cout][cin][3][3] -> dst, cout*cin*9*parts/2 floats (packed halves).
 * ksize 1 (descriptor: ksize 1, shuffle 1, algo 3): the decoder's pixel-shuffle GEMM -- ConvTranspose2d 2x2 (src0, C0, low
 * resolution) + the skip tensor (src1, C1, at the OUTPUT resolution) + 1x1 shortcut folded into one weight matrix
 * [4*cout][C0+C1] (archs/Unet.py:445-463, modules.py:163-196) -- in the same kernel, for (C0+C1) % 48 == 0 and cout % 64 == 0. */
int yond_conv_split_supported(int ksize, int stride, int cin, int cout);
int yond_pack_conv_split_weight_f32(const float* w, int cout, int cin, int ksize, int tn, int parts, float* dst);
/* 1 if the decoder GEMM described by `desc` (filled in for algo 3) may run with algo = 6 instead (csrc/gemm_k1_stationary.hip), else 0. */
int yond_gemm_k1_stationary_supported(const YondConvDesc* desc);
/* 1 if the stride-2 layer described by `desc` (filled in for algo 3) may run with algo = 7 instead (csrc/conv_s2_tall.hip), else 0. */
int yond_conv_s2_tall_supported(const YondConvDesc* desc);
/* Which instantiation of the split-operand kernel yond_conv2d_f32 launches for `desc` (algo 3 or 4): its index in the table of variants
 * (csrc/conv_split_kernel.h), or the negative error code the launch would return.  Host arithmetic on the descriptor's numbers only: no pointer is
 * dereferenced, no GPU needed.  yond_conv_split_variant_name: the variant's name (its tile, operands, staging, output and extras), NULL outside the table. */
int yond_conv_split_variant(const YondConvDesc* desc);
const char* yond_conv_split_variant_name(int variant);
/* The same packing on the device (w and dst are device pointers; asynchronous on `stream`): the training step re-packs the
 * weights it has just updated without a host round trip.  A weight outside fp16's range sets bit 0 of *status (device int,
 * may be NULL) instead of failing the call. */
int yond_pack_conv_split_weight_dev_f32(const float* w, int cout, int cin, int ksize, int tn, int parts, float* dst, int* status,
                                        void* stream);
/* The same for several layers in one launch (a training step re-packs every layer): desc (device) holds 7 int64 per layer -- source
 * offset in src (floats), cout, cin, taps (ksize^2), tn, destination offset in dst (floats), index of the layer's first 16-byte
 * group among all layers' groups (cout * cin * taps / 4 groups per layer at parts = 2); ngroups = their total. */
int yond_pack_conv_split_weights_batch_dev_f32(const float* src, const long long* desc, int nlayers, float* dst, size_t ngroups,
                                               int* status, void* stream);

/* First layer: 3x3, Cin=4 -> Cout=32k, input NHWC4, optional division by the per-image maximum
 * (data_normalize, archs/Unet.py:427-431) and LeakyReLU(slope).  wpk from yond_pack_conv_in_weight_f32. */
int yond_conv_in_f32(const float* x, const float* ub /*[N] or NULL*/, int N, int H, int W, int Cout,
                     const float* wpk, const float* bias, float slope, float* dst,
                     int out_fmt /* YOND_FMT_NHWC_F32: [N][H][W][Cout]; YOND_FMT_PLANES4: [N][Cout/4][H*W][4] */, void* stream);
int yond_pack_conv_in_weight_f32(const float* w /*[cout][4][3][3]*/, int cout, float* dst /*cout*40*/);

/* Last layer: 1x1 Cin -> 4, + x/ub residual, * ub (archs/Unet.py:463-468). */
int yond_conv_out_f32(const float* feat /*[N][H][W][Cin]*/, int Cin, const float* w /*[4][Cin]*/,
                      const float* bias /*[4]*/, const float* x /*[N][H][W][4] or NULL*/,
                      const float* ub /*[N] or NULL*/, int N, int H, int W, float* dst /*[N][H][W][4]*/,
                      void* stream);

/* Last layer of a plain convolution stack (DnCNN, archs/comp.py:24-32): 3x3, stride 1, zero padding, Cin -> 4,
 *   dst = x + sign * (conv3x3(feat) + bias),   sign = +1 or -1 (YOND_EINVAL otherwise); x NULL: dst = sign * (conv + bias).
 * fp32 operands, fp32-exact products on v_mfma_f32_4x4x1_16b_f32 (no operand is rounded to half: no range precondition, no status
 * word), fp32 accumulation: per output and tap column one chain of 3 * Cin fused multiply-adds, then the three columns, the bias
 * and the residual added in that order.  Cin % 16 == 0, Cin <= 128 (YOND_EUNSUPPORTED otherwise).  wpk from
 * yond_pack_conv3x3_out4_weight_f32: w OIHW [4][cin][3][3] -> dst, 36 * cin floats.
 * Non-finite inputs: as for algo 0 above -- an output is finite whenever its own 3 x 3 x Cin footprint (and its x) is. */
int yond_conv3x3_out4_f32(const float* feat /*[N][H][W][Cin]*/, int Cin, const float* wpk, const float* bias /*[4] or NULL*/,
                          const float* x /*[N][H][W][4] or NULL*/, float sign, int N, int H, int W, float* dst /*[N][H][W][4]*/,
                          void* stream);
int yond_pack_conv3x3_out4_weight_f32(const float* w /*[4][cin][3][3]*/, int cin, float* dst /*36*cin*/);

/* ------------------------------------------------------------------------------------------------
 * FBI_Net (archs/comp.py:264-648, case 'FBI_Net'): a blind-spot denoiser on the one-channel Bayer mosaic (csrc/fbinet.hip).
 * Activations are [N][H][W][nf] float32 at mosaic resolution (H = 2 h, W = 2 w of the packed frame), nf = 32 or 64.  Every product
 * is an exact fp32 product (the fp32-input MFMA, fmaf in the two edge kernels) with fp32 accumulation: no operand is rounded to half,
 * there is no range precondition and no status word.  Every entry returns YOND_EINVAL on a NULL pointer it needs and on shapes it
 * does not take, allocates nothing and runs on `stream`.  PReLU(x; s) = x > 0 ? x : s x, one slope per channel.
 *
 * yond_fbi_first_f32: n = PReLU(conv3x3 WITHOUT its centre tap (mosaic of x4, zero pad 1) + bias; slope[0]), 1 -> nf.  The mosaic
 *   pixel (y, x) is x4[y/2][x/2][2 (y&1) + (x&1)].  wpk from yond_pack_fbi_first_weight_f32 (w [nf][1][3][3] -> 8 * nf floats).
 * yond_fbi_tapconv_f32: n_out = PReLU(sum over the live taps t of W_t n_in(. + d_t) + bias; s1),  o_out = PReLU((n_out + o_in) / 2; s2),
 *   nf -> nf, zero border.  set 0: the 9 taps (0,1) (0,3) (1,0) (1,4) (2,2) (3,0) (3,4) (4,1) (4,3) of a 5x5 kernel, pad 2;
 *   set 1: centre and corners of a 3x3 kernel at dilation 3, pad 3.  wpk from yond_pack_fbi_tap_weight_f32 (w OIHW, unmasked:
 *   [nf][nf][5][5] or [nf][nf][3][3] -> yond_fbi_taps(set) * nf * nf floats: the dead taps are not read).  n_out and o_out must not
 *   be n_in.  yond_fbi_tile gives the pixel tile of a workgroup (tests place pixels on its seams).
 * yond_fbi_rm_f32: o = PReLU((v + W2 PReLU(W1 v + b1; a1) + b2) / 2; a2) on npix pixels, W1, W2 [nf][nf] packed by
 *   yond_pack_fbi_rm_weight_f32 (nf * nf floats each).  pre_slope != NULL: v is PReLU(v / pre_div; pre_slope) first (pre_div >= 1).
 *   o_out may be NULL when sum_mode != 0.  sum_mode 0: sum is not touched, 1: sum = o, 2: sum += o.  o_out must not be v.
 * yond_fbi_out_f32: y = W f + b, W [oc][nf], oc = 1 or 2; use_sigmoid: y0 = sigmoid_value * sigmoid(y0);
 *   oc 2: dst4 = y0 * x4 + y1 at the same packed position, oc 1: dst4 = y0. */
int yond_fbi_taps(int set);
int yond_fbi_tile(int* th, int* tw);
int yond_pack_fbi_first_weight_f32(const float* w, int nf, float* dst);
int yond_pack_fbi_tap_weight_f32(const float* w, int nf, int set, float* dst);
int yond_pack_fbi_rm_weight_f32(const float* w, int nf, float* dst);
int yond_fbi_first_f32(const float* x4 /*[N][h][w][4]*/, int N, int h, int w, int nf, const float* wpk, const float* bias /*[nf]*/,
                       const float* slope /*[1]*/, float* dst /*[N][2h][2w][nf]*/, void* stream);
int yond_fbi_tapconv_f32(const float* n_in, const float* o_in, int set, int nf, const float* wpk, const float* bias, const float* s1,
                         const float* s2, int N, int H, int W, float* n_out, float* o_out, void* stream);
int yond_fbi_rm_f32(const float* v, int nf, const float* w1p, const float* b1, const float* a1, const float* w2p, const float* b2,
                    const float* a2, const float* pre_slope /* or NULL */, int pre_div, size_t npix, float* o_out, float* sum, int sum_mode,
                    void* stream);
int yond_fbi_out_f32(const float* f /*[N][2h][2w][nf]*/, int nf, const float* w, const float* b, int oc, int use_sigmoid,
                     float sigmoid_value, const float* x4 /*[N][h][w][4]; oc 2 only*/, int N, int h, int w_, float* dst4 /*[N][h][w][4]*/,
                     void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Training FBI_Net (csrc/fbinet_train.hip): the backward entries the step needs beside the forward kernels above.  Same tensors
 * ([N][H][W][nf] float32, nf 32 | 64), same arithmetic: exact fp32 products (the fp32-input MFMA, or the exact float64 product of two
 * float32), nothing rounded to half.  Every sum over pixels goes through per-workgroup partial sums in `ws` (16-byte aligned, at least
 * yond_fbi_train_ws_bytes(nf, N, H, W) bytes: one workspace serves every entry at that shape) and a finish that adds them in float64
 * in workgroup order: no float atomics, two calls give the same bits.
 * yond_fbi_wgrad_f32: dwb = dW [taps][nf (co)][nf (ci)], then db [nf]:  dW_t[co][ci] = sum_{n,y,x} dz[n,y,x,co] x[n,y+dy_t,x+dx_t,ci]
 *   over the live taps of set 0 | 1 (yond_fbi_tapconv_f32's, in its order) or set 2, a 1x1 convolution (one tap); reads outside the
 *   frame are zero; db[co] = sum dz.  A workgroup accumulates yond_fbi_wgrad_rows(N, H) image rows (that many times W terms) in fp32.
 * yond_fbi_prelu_f32: u = (a + b) / div (b NULL: a / div; div >= 1), y = u > 0 ? u : slope u; slope_n = nf (per channel) or 1.
 *   u (may be NULL) receives the PReLU's input.
 * yond_fbi_prelu_bwd_f32: du = dy (u > 0 ? 1 : slope) / div -- the gradient of a and of b alike --, dslope [slope_n] = sum of dy u
 *   over u <= 0 (slope_n 1: over all channels).
 * yond_fbi_first_bwd_f32: the first layer's dwb = dW [8 live taps, yond_pack_fbi_first_weight_f32's order][nf], then db [nf], from
 *   dz [N][2h][2w][nf] and the packed batch x4.
 * yond_fbi_out_bwd_f32: the output layer (yond_fbi_out_f32's arguments) from dpred4 [N][h][w][4]: df [N][2h][2w][nf] and
 *   dwb [2 nf + 2] = dW row 0 [nf], dW row 1 [nf], db0, db1 (oc 1: row 1 and db1 are zero). */
size_t yond_fbi_train_ws_bytes(int nf, int N, int H, int W);
int yond_fbi_wgrad_rows(int N, int H);
int yond_fbi_wgrad_f32(const float* x, const float* dz, int set, int nf, int N, int H, int W, float* dwb, void* ws, size_t ws_bytes,
                       void* stream);
int yond_fbi_prelu_f32(const float* a, const float* b /* or NULL */, float div, const float* slope, int slope_n, int nf, size_t npix,
                       float* u /* or NULL */, float* y, void* stream);
int yond_fbi_prelu_bwd_f32(const float* u, const float* dy, float div, const float* slope, int slope_n, int nf, size_t npix, float* du,
                           float* dslope, void* ws, size_t ws_bytes, void* stream);
int yond_fbi_first_bwd_f32(const float* x4, const float* dz, int N, int h, int w, int nf, float* dwb, void* ws, size_t ws_bytes, void* stream);
int yond_fbi_out_bwd_f32(const float* f, int nf, const float* w, const float* b, int oc, int use_sigmoid, float sigmoid_value,
                         const float* x4, const float* dpred4, int N, int h, int w_, float* df, float* dwb, void* ws, size_t ws_bytes,
                         void* stream);

/* Minimum and maximum of the bias-corrected stabilised value that yond_pack_vst_norm_f32 / _biaslut_f32 / _batch_f32 normalise
 * (the same device function, float64), over each of B Bayer frames [B][H][W] that share the constants and the LUT:
 * out [B][2] float64 = (min, max) -- the reference's `lower, upper = raw_vst.min(), raw_vst.max()` of its 'fbi' branch
 * (YOND_SIDD.py:266-267).  lut_n 0: no bias; biaslut 0: the 1-D knots (lut_y float32), else the merged row of the 2-D table
 * (lut_y float64).  The reduction is on ordered integers: the result does not depend on the launch geometry. */
int yond_vst_minmax_f32(const float* bayer, int B, int H, int W, double scale, double gain, double sigma, const double* lut_x,
                        const void* lut_y, int lut_n, int biaslut, double* out /*[B][2]*/, void* stream);

/* 2x2 max pooling, NHWC (UNetSeeInDark, archs/Unet.py:60-72). */
int yond_maxpool2_f32(const float* src, int N, int H, int W, int C, float* dst, void* stream);

/* sigma-conditioning vectors for one GuidedResidualBlock / SNR_Block (archs/modules.py:170-178,190-193
 * / 205-214, 225-231), folded with the conv biases into the epilogue (scale, shift) pairs of conv1 and
 * conv2.  t: [N] (already divided by ub when ub != NULL is NOT assumed: the kernel divides).
 *   kind 0 GuidedResidualBlock: m1 = gamma (w_a0,b_a0,w_a2,b_a2), m2 = beta (w_b,b_b)
 *   kind 1 SNR_Block:           m1 = sfm1, m2 = sfm2 (w_b0,b_b0 used as second first-layer)
 * Outputs s1,t1,s2,t2: [N][ld], only the first C entries of a row are written (channel padding stays 0).
 * `descs` is a DEVICE array of nblocks descriptors. */
typedef struct YondFilmDesc {
    int kind, C, ld;                           /* C <= 1024 real channels; ld = row stride of the outputs */
    const float *w_a0, *b_a0, *w_a2, *b_a2;   /* first MLP: 1->C, C->C */
    const float *w_b0, *b_b0;                  /* SNR only: second MLP first layer 1->C */
    const float *w_b, *b_b;                    /* guided: beta C->C ; SNR: sfm2 second layer C->C */
    const float *cb1, *cb2;                    /* conv1 / conv2 biases [C] */
    float *s1, *t1, *s2, *t2;                  /* [N][ld] */
} YondFilmDesc;
int yond_film_f32(const YondFilmDesc* descs, int nblocks, const float* t /*[N]*/, const float* ub /*[N] or NULL*/,
                  int N, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K5  local statistics for the noise-level estimator (box means in float64, cv2.blur semantics:
 * normalised k x k window, BORDER_REFLECT_101, result rounded to float32).
 * Replaces utils/isp_algos.py:234-242 (stdfilt) and the cv2.blur calls at YOND_SIDD.py:67-71, 95-98.
 * All maps are planar packed [4][h][w]; `tile_w` > 0 makes every tile_w columns an independent image
 * (the SIDD_256 re-tiling of YOND_SIDD.py:64-65, 91-93), 0 means the whole width.
 *   stage 1 (self):   from Bayer: mean = B_k(x), var = stdfilt(x,k)^2, blur2 = B_k2(x)
 *   stage 2 (self):   from blur2: lap = stdfilt(blur2, k)
 *   collab:           from noisy & denoised Bayer: var = stdfilt(lr)^2 - stdfilt(hr)^2,
 *                     mean = B_k(hr), lap = stdfilt(hr) */
int yond_box_stats_self1_f32(const float* bayer, int H, int W, int k, int k2, int tile_w, float* mean,
                             float* var, float* blur2, void* stream);
int yond_box_stats_self2_f32(const float* blur2, int h, int w, int k, int tile_w, float* lap, void* stream);
int yond_box_stats_collab_f32(const float* bayer_lr, const float* bayer_hr, int H, int W, int k, int tile_w,
                              float* mean, float* var, float* lap, void* stream);

/* (K5' -- the same maps in ONE pass, the B19 map never leaving the chip -- measured slower than K5 + sweep 1 and was retired:
 * profiles/r05_experiments/README.md is the record, git history has the source.) */

/* K5+ the hot-path producers of the estimator, one call per frame: the streaming kernels of K5 (stage 1 of the self mode also
 * collects the frame maximum into the workspace head) followed by sweep 1 of the threshold selection (yond_nle_stats_f32
 * below) on the same workspace, which this call resets first.  `blur2` [4][H/2][W/2] is scratch
 * (the B19 map).  The default of SimpleNLF: fewer instructions per pixel than the retired K5' at 32 B/px more HBM traffic,
 * which the estimator (issue-bound, not HBM-bound) does not notice.  Any k that K5 takes. */
int yond_box_stats_self_stats_f32(const float* bayer, int H, int W, int k, int k2, int tile_w, float* mean, float* var,
                                  float* blur2, float* lap, const double* q_host, int nq, void* ws, void* stream);
int yond_box_stats_collab_stats_f32(const float* bayer_lr, const float* bayer_hr, int H, int W, int k, int tile_w,
                                    float* mean, float* var, float* lap, const double* q_host, int nq, void* ws, void* stream);

/* K6  exact order statistics of a non-negative float32 map (np.percentile's two neighbours).
 * ranks: nr 0-based ranks (device int64); out: nr float values (device).  ws: workspace of
 * yond_select_ws_bytes(nr) bytes.  Replaces the sort inside np.percentile at YOND_SIDD.py:26,80. */
size_t yond_select_ws_bytes(int nr);
int yond_select_ranks_f32(const float* data, size_t n, const int64_t* ranks_host, int nr, float* out, void* ws,
                          void* stream);
/* np.percentile(data, q, method='linear') (YOND_SIDD.py:26,80): q_host[nq] in percent (host array, nq <= 32),
 * out: nq float64 values (device).  Same workspace as yond_select_ranks_f32. */
int yond_percentiles_f32(const float* data, size_t n, const double* q_host, int nq, double* out, void* ws,
                         void* stream);

/* K6'/K7' the threshold selection of the estimator in two sweeps (YOND_SIDD.py:22-49: np.percentile at :26, the masked
 * bincounts at :37-43, score and argmin at :45-47), replacing yond_percentiles_f32 + yond_nlf_occupancy_f32 +
 * yond_nlf_score3_f64 on the hot path.  `ws`: device workspace of yond_nle_ws_bytes(n) bytes, 16-byte aligned.
 *   yond_nle_stats_f32      sweep 1 over (lap, mean) (n elements as rows of `width`): level-1 histogram of lap and, per
 *                           1/1000 mean bin, the smallest lap (a bin is occupied among lap <= T iff its smallest lap <= T);
 *                           resets the workspace first.
 *   yond_nle_threshold_f32  sweep 2 over lap + finish: the exact order statistics, np.percentile(lap, q, 'linear') ->
 *                           ths; with want_score: npeaks[i], score = ths / (q * npeaks), i* = argmin(score[1:]) + 1 -> sel.
 *                           Needs sweep 1's state in `ws`; may be repeated on it (its own counters are reset when it ends).
 *   Results stay in the head of the workspace: yond_nle_state_layout gives the byte offsets of
 *   {ths double[32], sel double[4] = {i*, ths[i*], q[i*], score[i*]}, mom double[10], npeaks int32[32], frame_max_key};
 *   yond_nlf_moments_f32 can take th = ws + off[1] + 8 and mom = ws + off[2] directly. */
size_t yond_nle_ws_bytes(size_t n);
int yond_nle_stats_f32(const float* lap, const float* mean, size_t n, int width, const double* q_host, int nq, void* ws,
                       void* stream);
int yond_nle_threshold_f32(const float* lap, size_t n, const double* q_host, int nq, int want_score, void* ws, void* stream);
int yond_nle_state_layout(int* off /*[5]*/);
/* K7b on that workspace: the moment sums below sel[1] are ADDED to the workspace's mom, which the reset of sweep 1 zeroed (no
 * memset launch of its own): ONE call per sweep 1 -- a second call on the same state would double the sums (use
 * yond_nlf_moments_f32, which zeroes its destination, for anything else). */
int yond_nle_moments_f32(const float* lap, const float* mean, const float* var, size_t n, void* ws, void* stream);

/* K7a occupancy: one pass over (lap, mean), n elements laid out as rows of `width` (n % width == 0; pass the
 *   image row length so that a lane can walk down a column of the smooth maps; any width is correct):
 *   for thresholds ths[0..nt) (ascending, float64, device)
 *   occ  [nt][32] uint32 bitmap: bit (bin & 31) of word bin >> 5 set when bin floor(clip(mean,0,1)*1000) is
 *        occupied among {ths[i-1] < lap <= ths[i]}   (YOND_SIDD.py:37-43; prefix-OR over i gives npeaks) */
int yond_nlf_occupancy_f32(const float* lap, const float* mean, size_t n, int width, const double* ths, int nt,
                           uint32_t* occ, void* stream);

/* K7s score3 on the device (YOND_SIDD.py:37-47): npeaks[i] = number of bins occupied among lap <= ths[i],
 *   score = ths / (quants * npeaks) in float64, i* = argmin(score[1:]) + 1.
 *   quants_host: nt float64 on the host.  sel (device, 4 float64): {i*, ths[i*], quants[i*], score[i*]};
 *   npeaks (device, nt int32). */
int yond_nlf_score3_f64(const uint32_t* occ, const double* ths, const double* quants_host, int nt, double* sel,
                        int32_t* npeaks, void* stream);

/* K7b moments: one pass over (lap, mean, var): mom [2][5] float64 = {n, sum m, sum v, sum m^2, sum m v} over
 *   {lap < *th}, [0] all pixels, [1] only 1e-4 < mean < 0.8 (YOND_SIDD.py:77, 105; utils/isp_algos.py:348-350,
 *   352-364 as moment sums).  th: one float64 on the device (e.g. sel + 1 of yond_nlf_score3_f64). */
int yond_nlf_moments_f32(const float* lap, const float* mean, const float* var, size_t n, const double* th,
                         double* mom, void* stream);

/* Row H  bias LUT construction on the device (utils/isp_algos.py:49-140): for every knot lam <= th the
 * Poisson (*) Gaussian expectation of the VST, above th Foi's closed form.  lams: float64[n] (device),
 * bias: float32[n] (device out). */
int yond_bias_lut_f64(const double* lams, int n, double gain, double sigma, float* bias, void* stream);

/* N1  per-block PSNR / SSIM partial sums (YOND_SIDD.py:649-652, 679-697).  dn, hr: Bayer [H][W]; blocks of
 * bh x bw (row-major block order); out: [nblocks][ntiles][2] float64 = {sum of squared error, sum of SSIM
 * over the 'valid' map} per 32x32 tile, ntiles = yond_block_metrics_tiles(bh, bw); the host adds the tiles:
 * psnr = 10 log10(1 / (sum_se / (bh*bw))), ssim = sum_ssim / ((bh-10)*(bw-10)).
 * Blocks smaller than 11 x 11 (no 'valid' position) are YOND_EINVAL.  The tiles of a block are one grid dimension of the launch: a block
 * of more than 65,535 tiles (beyond about 8,160 x 8,160) is refused -- yond_block_metrics_tiles returns YOND_EUNSUPPORTED, and
 * yond_block_metrics_f32 returns the same before it launches anything. */
int yond_block_metrics_tiles(int bh, int bw);
int yond_block_metrics_f32(const float* dn, const float* hr, int H, int W, int bh, int bw, double* out,
                           void* stream);

/* N1 on sRGB codes (YOND_SIDD.py:657-677, 712-717 calculate_ssim on a three-channel image).  dn, hr: interleaved uint8 [H][W][3];
 * out: [nblocks][ntiles][3][2] float64 = per channel {sum of squared code error, sum of SSIM over the 'valid' map} per 32x32 tile.
 * The same kernel as yond_block_metrics_f32 on a uint8 loader: the codes ARE the [0,255] values (no x255), same window, C1, C2 and
 * refusals.  The host adds the tiles: psnr_rgb = 10 log10(255^2 / (sum_se over the 3 channels / (3*bh*bw))), ssim_rgb = the mean
 * of the three channels' sum_ssim / ((bh-10)*(bw-10)). */
int yond_block_metrics_rgb8(const unsigned char* dn, const unsigned char* hr, int H, int W, int bh, int bw, double* out,
                            void* stream);

/* R1  raw Bayer frame -> sRGB (isp.hip; utils/sidd_utils.py:156-277 process_sidd_image, utils/isp_ops.py:171-197 FastISP).
 *   frame      float32 (device): layout YOND_ISP_BAYER [H][W], or YOND_ISP_PACKED4 [H/2][W/2][4] in R, G1, G2, B order; H, W even
 *   flip_lr/ud the frame is read mirrored (flip_bayer, sidd_utils.py:182-196: brings the pattern to RGGB); Bayer layout only
 *   gains      float64 [4] (host), one per CFA site of the RGGB frame (R, G1, G2, B)
 *   ccm        float64 [9] (host), row-major camera -> sRGB matrix
 *   mode       YOND_ISP_SIDD: clip(0,1), float32 x float64 gain in float64, clip(0,1), x16383.0, clip, truncate; the demosaiced
 *              integer / 16383 is a float32 division.  YOND_ISP_FAST: the gained value is rounded to float32 (FastISP stages the
 *              frame in float32), clipped, x16383 in float32, truncated; the quotient is a float64 division.
 *   demosaic   on the integers, RGGB, neighbours outside the frame mirrored without repeating the edge (-1 -> 1, H -> H-2).  R / B
 *              site: own colour = q; G = (up+down+1)>>1 if |left-right| > |up-down| else (left+right+1)>>1; the opposite colour =
 *              (four diagonals + 2)>>2.  G site: the horizontal neighbours' colour = (left+right+1)>>1, the other = (up+down+1)>>1.
 *              This is the project's restatement of cv2's COLOR_BayerBG2RGB_EA: UNPINNED.
 *   colour     x_r = (d0*M[r][0] + d1*M[r][1]) + d2*M[r][2] in float64, no contraction, then clip(0,1)
 *   out_u8     (nullable, 4-byte aligned) uint8 [H][W][3], order YOND_ISP_RGB or YOND_ISP_BGR: code = #{k in 1..255 : thresholds[k-1]
 *              <= x}, thresholds float64 [255] (device) = (k/255)^2.2 -- trunc(max(x,1e-8)^(1/2.2) * 255) away from the thresholds
 *   out_f32    (nullable) float32 [H][W][3] RGB = x^(1/gamma), pow in float64 rounded once
 * Refused (YOND_EINVAL, nothing launched): a null frame / gains / ccm, H or W odd or < 2, both outputs null, out_u8 without
 * thresholds or misaligned, an unknown layout / mode / order, flips with the packed layout, gamma <= 0 with out_f32. */
#define YOND_ISP_BAYER 0
#define YOND_ISP_PACKED4 1
#define YOND_ISP_SIDD 0
#define YOND_ISP_FAST 1
#define YOND_ISP_RGB 0
#define YOND_ISP_BGR 1
int yond_render_srgb(const float* frame, int H, int W, int flip_lr, int flip_ud, int layout, const double* gains, const double* ccm,
                     int mode, const double* thresholds, unsigned char* out_u8, int order, float* out_f32, double gamma, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The per-frame parameter chain on the device: no host round trip between the estimator and the network.
 * Replaces the host arithmetic of YOND_SIDD.py:341-356 (beta -> K, sigma), :438-447 (round-2 guards), :263-264, 284-285
 * (lower = VST(0), upper = VST(scale), t = 1.03 / (upper - lower)), utils/isp_algos.py:101-108 (knot grid of get_bias)
 * and :345-365 (polyfit on the moment sums).
 * yond_frame_params_f64: reads the estimator's workspace (after yond_nle_moments_f32) and writes
 *   prm[YOND_PRM_N]   the parameter block below (float64),
 *   t_out             the network's noise level as float32 (or NULL),
 *   lut_x[lut_cap]    the knot grid of get_bias for the frame maximum (max_dev: a float32 device scalar, or NULL: the
 *                     maximum the estimator's first kernel collected).
 * mode 0: round 1 (:356), 1: round 2 (:438-447).  Branches that need more work than this chain does are FLAGGED in
 * prm[YOND_PRM_FLAGS] and left to the caller (host path): no flat area, knot capacity, K <= 0.
 * The *_dev_* entry points below take gain / sigma / lower / upper / the LUT size from such a block. */
#define YOND_PRM_BETA1 0
#define YOND_PRM_BETA2 1
#define YOND_PRM_GAIN 2
#define YOND_PRM_SIGMA 3
#define YOND_PRM_LO 4
#define YOND_PRM_HI 5
#define YOND_PRM_NSR 6
#define YOND_PRM_T 7          /* float32 value of the network's t */
#define YOND_PRM_FLAGS 8      /* YOND_PRM_FLAG_* as a number */
#define YOND_PRM_LUT_N 9
#define YOND_PRM_NSEL 10      /* pixels below the selected threshold */
#define YOND_PRM_TH 11
#define YOND_PRM_PCT 12
#define YOND_PRM_FRAME_MAX 13
#define YOND_PRM_N 16
#define YOND_PRM_FLAG_NO_FLAT_AREA 1   /* YOND_SIDD.py:79-84: the 25 % fallback needs the host path */
#define YOND_PRM_FLAG_LUT_CAPACITY 2   /* more knots than lut_cap (or more LDS than the LUT kernel has) */
#define YOND_PRM_FLAG_ROUND_ABORTED 4  /* round 2: beta1 < 0 (:445-447): the caller drops this round's output */
#define YOND_PRM_FLAG_BAD_ESTIMATE 8   /* K <= 0 or NaN: nothing downstream is defined */
int yond_frame_params_f64(const void* nle_ws, const float* max_dev, int mode,
                          double scale_est /* wp - bl: beta -> (K, sigma) in DN, :356 */, double scale /* p['scale'] = (wp - bl) / ratio: the VST's DN scale, :251 */,
                          double tfac, int lut_cap, double* prm, float* t_out, double* lut_x, void* stream);
/* The frame chain as ONE launch: yond_frame_params_f64 + yond_bias_lut_dev_f64 + yond_lut_table_f64 (same block, knots, ordinates,
 * table and flags).  Every workgroup derives the parameters itself, integrates one knot, and the last to arrive writes the table.
 * nle_ws: the estimator's workspace after yond_nle_moments_f32 (its arrival counter, word 2 of the state's tickets, is left at zero);
 * lut_y [lut_cap] float32, lut_ws yond_lut_ws_bytes(lut_cap) bytes. */
int yond_frame_chain_f64(void* nle_ws, const float* max_dev, int mode, double scale_est, double scale, double tfac, int lut_cap,
                         double* prm, float* t_out, double* lut_x, float* lut_y, void* lut_ws, void* stream);
/* Row H for large K * sigma (14-bit sensors at a digital gain: the Gaussian table of the integration exceeds the LDS and
 * yond_bias_lut_f64 returns YOND_EUNSUPPORTED): the same integration with the table in a caller-provided scratch buffer of
 * yond_bias_lut_big_scratch(gain, sigma, nwg) doubles, nwg workgroups striding over the knots.  Seconds, not microseconds. */
size_t yond_bias_lut_big_scratch(double gain, double sigma, int nwg);
/* get_bias_points (utils/isp_algos.py:142-160; BiasLUT.get_lut's pointwise branch :210-212 calls it with pho_min = 100,
 * close_form = True): the integration at ARBITRARY abscissae lams[n], sampling rate max(int(sqrt K), pho_min), Foi's closed
 * form above th only with close_form (else every point is integrated; pass lam_max = max(lams)).  Output float32 (bias32)
 * or float64 (bias64), scratch of yond_bias_points_scratch(...) doubles. */
size_t yond_bias_points_scratch(double gain, double sigma, int pho_min, int close_form, double lam_max, int nwg);
int yond_bias_points_f64(const double* lams, int n, double gain, double sigma, int pho_min, int close_form, double lam_max,
                         float* bias32, double* bias64, double* scratch, size_t scratch_doubles, int nwg, void* stream);
int yond_bias_lut_big_f64(const double* lams, int n, double gain, double sigma, float* bias, double* scratch,
                          size_t scratch_doubles, int nwg, void* stream);
/* Row H with (n, K, sigma) read from the block: launches lut_cap workgroups, those beyond prm[LUT_N] exit. */
int yond_bias_lut_dev_f64(const double* lams, int lut_cap, double* prm, float* bias, void* stream);
/* The LUT in the form K1 evaluates (per-interval coefficients + run table), prepared ONCE per frame instead of once per
 * workgroup of K1: lut_ws must hold yond_lut_ws_bytes(lut_cap) bytes.  n < 0: the size comes from prm. */
size_t yond_lut_ws_bytes(int lut_cap);
int yond_lut_table_f64(const double* lut_x, const float* lut_y, int n, const double* prm /* n < 0: also receives a flag */, void* lut_ws, void* stream);
/* K1 / K4 with the frame's constants in a parameter block and the LUT as a prepared table. */
int yond_pack_vst_norm_dev_f32(const float* bayer, int H, int W, float* out, int pad_l, int pad_r, int pad_t, int pad_b,
                               double scale, const double* prm, const void* lut_ws /* NULL: no bias correction */,
                               int lut_cap /* the capacity lut_ws was prepared for */, float* img_max, void* stream);
/* K1 of the device chain proper: as yond_pack_vst_norm_dev_f32 for the table yond_frame_chain_f64 / yond_lut_table_f64 prepared from
 * get_bias' knot grid (<= 3 evenly spaced runs of non-zero width), with the affine tail of the normalisation folded into the table's coefficients
 * (6 float64 operations per element instead of 11; the float32 result differs from yond_pack_vst_norm_dev_f32's for about one element
 * in 1e8, by one ulp).  prm is also written: a table of another shape sets YOND_PRM_FLAG_LUT_CAPACITY and nothing is computed. */
int yond_pack_vst_norm_chain_f32(const float* bayer, int H, int W, float* out, int pad_l, int pad_r, int pad_t, int pad_b,
                                 double scale, double* prm, const void* lut_ws, int lut_cap, float* img_max, void* stream);
int yond_denorm_ivst_unpack_dev_f32(const float* net_out, int Hp, int Wp, int pad_t, int pad_l, int h, int w, float* bayer,
                                    int mode, double scale, const double* prm, int clip01, void* stream);
/* K1 / K4 of the device chain for B equally sized frames that share the parameter block and the table (the 32 blocks of a SIDD image,
 * YOND_SIDD.py:392-407): bayer [B][H][W] -> out [B][Hp][Wp][4], img_max [B];  net_out [B][Hp][Wp][4] -> bayer_out [B][2h][2w]. */
int yond_pack_vst_norm_batch_dev_f32(const float* bayer, int B, int H, int W, float* out, int pad_l, int pad_r, int pad_t, int pad_b,
                                     double scale, const double* prm, const void* lut_ws, int lut_cap, float* img_max, void* stream);
int yond_denorm_ivst_unpack_batch_dev_f32(const float* net_out, int B, int Hp, int Wp, int pad_t, int pad_l, int h, int w,
                                          float* bayer_out, int mode, double scale, const double* prm, int clip01, void* stream);

/* ------------------------------------------------------------------------------------------------
 * N4, first slice: what one training step needs beyond the forward kernels (trainer_AWGN.py:101-117, losses/base_loss.py:81-113,
 * torch.optim.Adam).  Data gradients run on yond_conv2d_f32 with re-indexed weights (yond_public_amd/train.py).
 * yond_conv_wgrad_f32: dw[tap][Cout][Cin] = sum_p dy[p_out][Cout] x[p_in(p_out, tap)][Cin] on the fp32 MFMA (Cin, Cout
 *   multiples of 32, NHWC); mode 0: 3x3 pad 1 (stride 1 / 2: Ho = ceil(H / stride)), 1: ConvTranspose2d 2x2 stride 2
 *   (Ho = 2H; taps dy*2+dx), 2: 1x1.
 * yond_colsum_f32: db[c] = sum_p dy[p][c].   yond_l1_loss_f32: loss_sum = sum |pred - target|, grad = sign(.) / n.
 * yond_adam_step_f32: torch.optim.Adam's single-tensor update (no weight decay / amsgrad), step = 1, 2, ...
 *   m' = m + w1 (g - m), v' = v b2 + (g g) w2, p' = p - step_size (m' / (sqrt(v') inv_bc2_sqrt + eps)): one float32 rounding per
 *   operation, no FMA.  Every scalar is formed in float64 and rounded to float32 once, as torch rounds the doubles it hands to
 *   lerp_ / addcmul_: w1 = float32(1 - beta1), w2 = float32(1 - beta2) (NOT 1.0f - float32(beta): 1.29e-5 apart for beta2 = 0.999),
 *   b2 = float32(beta2), step_size = float32(lr / (1 - beta1^step)), inv_bc2_sqrt = float32(1 / sqrt(1 - beta2^step)), eps.  The
 *   stored state is torch's up to the order of roundings (torch's kernels fuse each state line into one FMA): tests/train_model.py
 *   has the float64 model and the per-element bounds.  Any element alignment.
 * Losses with a NaN in pred or target: loss_sum becomes NaN (what TrainStep's third status word reports; the update is skipped); the
 *   gradient at that element is 0 from yond_l1_loss_f32 (neither comparison holds) and NaN from yond_charbonnier_loss_f32; every
 *   other element is unaffected.  pred == target (d = +-0) gives the L1 gradient +0.  The gradient scale is 1.0f / (float)n. */
int yond_conv_wgrad_f32(const float* x, const float* dy, int N, int H, int W, int Cin, int Ho, int Wo, int Cout, int mode,
                        int stride, float* dw, void* stream);
/* The same with a workspace: ws (device, yond_conv_wgrad_ws_bytes(...) bytes) takes the workgroups' partial sums, which a second
 * kernel adds up -- the K axis (pixels) is split over thousands of waves, and float atomics onto the few addresses of a
 * low-channel layer serialise at the memory side.  ws NULL: atomics, as yond_conv_wgrad_f32. */
size_t yond_conv_wgrad_ws_bytes(int N, int H, int W, int Cin, int Ho, int Wo, int Cout, int mode, int stride);
int yond_conv_wgrad_ws_f32(const float* x, const float* dy, int N, int H, int W, int Cin, int Ho, int Wo, int Cout, int mode, int stride,
                           float* dw, float* ws, size_t ws_bytes, void* stream);
/* The weight gradient of a 3x3 stride-1 pad-1 layer on the fp16 matrix cores with fp32-accurate split operands (csrc/wgrad_split.hip;
 * the pixel axis is the MFMA's K axis, both tensors staged as fp16 halves and read transposed from LDS).  dw as above
 * ([9][Cout][Cin]); needs |dy| < 32 (bit 0 of *status is set otherwise: TrainStep's loss scale keeps it there).
 * yond_conv_wgrad_split_ws_bytes returns 0 for a layer the kernel does not take (the caller keeps yond_conv_wgrad_ws_f32). */
size_t yond_conv_wgrad_split_ws_bytes(int N, int H, int W, int Cin, int Cout);
/* Read-only: the geometry yond_conv_wgrad_split_f32 would run this layer with -- out[0] the tile configuration (1..5; 0: the layer is
 * not taken and the other four are 0), out[1] the number of K slices, out[2] the steps per slice, out[3] the X ring's pixels, out[4]
 * the dynamic LDS bytes.  Host only, no launch (tests assert the geometry a case reaches).  YOND_EINVAL for a null out. */
int yond_conv_wgrad_split_plan(int N, int H, int W, int Cin, int Cout, int out[5]);
int yond_conv_wgrad_split_f32(const float* x, const float* dy, int N, int H, int W, int Cin, int Cout, float* dw,
                              int with_bias /* bit 0: dw has 9 Cout Cin + Cout floats, the last Cout = db[co] = sum_p dy[p][co];
                                               bit 1: the weight gradient in OIHW order, dw[co][ci][tap] */,
                              float* ws, size_t ws_bytes, int* status, void* stream);
int yond_colsum_f32(const float* dy, size_t npix, int C, float* db, void* stream);
/* The guided block's middle (archs/modules.py:186-196) for training: out = SiLU(z * tk[n][c] + tb[n][c]) over z [N][P][C] with
 * per-image vectors tk, tb [N][C], and its backward in one pass: dz, dtk[n][c] = sum_p g z, dtb[n][c] = sum_p g with
 * g = dout * SiLU'(z tk + tb).  C in {32, 64, 128, 256, 512, 1024} (yond_film_silu_supported); other widths stay with the caller. */
int yond_film_silu_supported(int C);
int yond_film_silu_f32(const float* z, const float* tk, const float* tb, float* out, int N, size_t P, int C, void* stream);
int yond_film_silu_bwd_f32(const float* z, const float* tk, const float* tb, const float* dout, float* dz, float* dtk, float* dtb, int N,
                           size_t P, int C, void* stream);
/* The sigma-conditioning MLPs of a guided block for training (archs/modules.py:170-178): a = t w1 + b1, h = SiLU(a), tk = W2 h + b2,
 * tb = W3 SiLU(tk) + b3 for t [B]; w1, b1, b2, b3 [C]; W2, W3 [C][C] (Conv2d 1x1 weights).  fwd writes tk, tb at row stride ld >= C
 * (zero beyond C).  bwd: from the gradients dtk, dtb (row stride ld) the parameter gradients; scratch
 * 2 B C floats.  yond_silu_bwd_add_f32: dx = dres + dz SiLU'(x) (a residual block's input gradient in one pass). */
int yond_film_mlp_fwd_f32(const float* t, const float* w1, const float* b1, const float* W2, const float* b2, const float* W3,
                          const float* b3, int B, int C, int ld, float* tk, float* tb, void* stream);
int yond_film_mlp_bwd_f32(const float* t, const float* w1, const float* b1, const float* W2, const float* W3, const float* tk,
                          const float* dtk, const float* dtb, int B, int C, int ld, float* scratch, float* dw1, float* db1,
                          float* dW2, float* db2, float* dW3, float* db3, void* stream);
/* The same for ALL guided blocks of a network at once (n <= 12; the MLPs depend on sigma and the weights only): 2 launches forward,
 * 5 backward, instead of that many per block.  d: HOST array.  Forward reads t, w1 .. b3 and writes tk, tb ([B][ld]; columns beyond C
 * must already be zero); backward reads t, w1, b1, W2, W3, tk, dtk, dtb, uses scratch (2 * B * C floats) and writes dw1 .. db3. */
/* The plain GEMMs of a training step on the fp16 matrix cores with fp32-accurate split operands (csrc/gemm_split.hip): 1x1 convolutions
 * over one or two sources, their data gradients, ConvTranspose2d 2x2 (pixel-shuffle store) and its data gradient
 * (archs/Unet.py:447-461, archs/modules.py:142-147; backward of trainer_AWGN.py:116):
 *     y[p][n] = sum_s sum_k x_s[p][k] * B_s(k, n) (+ bias[n % nblk]),
 *     B_s(k, n) = w_s[(k % kblk) sk_lo + (k / kblk) sk_hi + (n % nblk) sn_lo + (n / nblk) sn_hi], zero where k % kblk >= k_real or n % nblk >= n_real
 * -- the float32 parameter itself, read through strides and split when staged (no packing pass).  x_s: [P][ld] float32, k (a multiple
 * of 32) channels taken; y: [P][ldy], n_p (a multiple of 32) channels written; shuffle != 0: y is [N][2H][2W][ldy], P = N H W,
 * n = j (n_p / 4) + co goes to pixel (2 yy + j / 2, 2 xx + j % 2), channel co (nblk must be n_p / 4).
 * status (may be NULL): TWO words -- bit 0 of status[0] is set when a staged x is NaN or beyond fp16's range (|x| > 65504), bit 0 of status[1]
 * when a weight is NaN or |w| >= 32 (the 2^11 w part leaves fp16's range).  (ABI 7; version 6 took one word, the weights'.) */
typedef struct YondGemmSrc {
    const float* x;
    const float* w;
    long long sk_lo, sk_hi;
    int ld, k, kblk, k_real;
} YondGemmSrc;
int yond_gemm_split_f32(const YondGemmSrc* src /* host array */, int nsrc /* 1 or 2 */, size_t P, int n_p, int n_real, long long sn_lo, long long sn_hi,
                        int nblk, const float* bias /* or NULL */, float* y, int ldy, int shuffle, int H, int W, int* status, void* stream);
typedef struct YondFilmMlpDesc {
    const float *t, *w1, *b1, *W2, *b2, *W3, *b3;
    float *tk, *tb;
    const float *dtk, *dtb;
    float* scratch;
    float *dw1, *db1, *dW2, *db2, *dW3, *db3;
    int B, C, ld, pad_;
} YondFilmMlpDesc;
int yond_film_mlp_fwd_multi_f32(const YondFilmMlpDesc* d, int n, void* stream);
int yond_film_mlp_bwd_multi_f32(const YondFilmMlpDesc* d, int n, void* stream);
/* dx = dres + dz SiLU'(x), n (a multiple of 4) floats.  This entry and yond_silu_f32 move float4: every pointer must be 16-byte aligned
 * (YOND_EINVAL otherwise; the other float4 kernels of this section -- colsum, film_silu, zero_interleave -- assume it).  SiLU and SiLU' are
 * u s and s (1 + u (1 - s)) with s = 1 / (1 + expf(-u)): below u = -88.72284 expf overflows, s = 0 and both return -0 where the true value
 * is below 3e-37 in magnitude. */
int yond_silu_bwd_add_f32(const float* x, const float* dz, const float* dres, float* dx, size_t n, void* stream);
/* y = SiLU(x), n (a multiple of 4) floats. */
int yond_silu_f32(const float* x, float* y, size_t n, void* stream);
/* g [N][H][W][C] = dy [N][ceil(H/2)][ceil(W/2)][C] at the even pixels, 0 elsewhere (the stride-2 layers' data gradient runs as a
 * stride-1 convolution over it). */
int yond_zero_interleave_f32(const float* dy, int N, int Ho, int Wo, int C, int H, int W, float* g, void* stream);
int yond_l1_loss_f32(const float* pred, const float* target, size_t n, double* loss_sum, float* grad /* or NULL */, void* stream);
/* L1_Charbonnier_loss (losses/base_loss.py:69-79; Unet_Loss(charbonnier=True), :82-85): loss_sum = sum sqrt(diff^2 + eps),
 * grad = diff / sqrt(diff^2 + eps) / n in the float32 steps of torch's backward */
int yond_charbonnier_loss_f32(const float* pred, const float* target, size_t n, double eps, double* loss_sum, float* grad /* or NULL */,
                              void* stream);
int yond_adam_step_f32(float* p, const float* g, float* m, float* v, size_t n, double lr, double beta1, double beta2, double eps,
                       int step, void* stream);
/* The same with the step's scalars on the device (hyp[0] = lr / (1 - beta1^step), hyp[1] = 1 / sqrt(1 - beta2^step) as float32), for a
 * step captured in a hipGraph; status (three int words, optional): no update when bit 0 of any is set (the kernels' two range words and one
 * of the caller's, e.g. a non-finite loss). */
int yond_adam_step_dev_f32(float* p, const float* g, float* m, float* v, size_t n, double beta1, double beta2, double eps,
                           const float* hyp, const int* status, void* stream);
/* Training-mode BatchNorm2d + ReLU and its backward (csrc/bn_train.hip; DnCNN's middle layers, archs/comp.py:18-26) on y [M][C] float32 --
 * an [N][H][W][C] tensor with M = N H W values per channel.  Four entries, six launches, no allocation, no float atomics: every result is
 * bitwise reproducible from run to run.
 *   yond_bn_stats_f32       Sy = sum y, Syy = sum y y per channel in float64 (workgroup partials in ws, added in a fixed order by a finish
 *                           launch), then  mean = Sy / M,  var = max(Syy / M - mean^2, 0) (biased),  rstd = 1 / sqrt(var + eps),
 *                           scale = gamma rstd,  shift = beta - mean scale -- all in float64, each rounded to float32 once.
 *                           stat [4][C]: mean, rstd, scale, shift.   pending [2][C]: the running statistics this batch WOULD leave,
 *                           (1 - momentum) running_mean + momentum mean  and  (1 - momentum) running_var + momentum var M / (M - 1)
 *                           (momentum: torch's, the weight of the new value; formed in float64, rounded once).  running_mean / running_var
 *                           are only read: the caller commits `pending` once the step's verdict is in.
 *   yond_bn_apply_relu_f32  out = max(fmaf(y, scale, shift), 0); a NaN stays a NaN (torch's ReLU).
 *   yond_bn_bwd_reduce_f32  with g = dout [fmaf(y, scale, shift) > 0] and yh = (y - mean) rstd (two float32 roundings):
 *                           dbeta = sum g, dgamma = sum g yh, float64 partials (g yh is exact there), fixed order, rounded to float32 once.
 *   yond_bn_bwd_apply_f32   dy = scale * fmaf(-yh, float32(dgamma / M), g - float32(dbeta / M))   (the divisions in float64).
 * The ReLU mask of the two backward entries is RECOMPUTED from (y, scale, shift) with the forward's own fmaf -- the same instruction on the
 * same three float32 values, so it is the forward's mask element for element -- not stored.
 * ws: yond_bn_train_ws_bytes(M, C) bytes, 8-byte aligned, fully overwritten by each reducing entry (stats and bwd_reduce may share it in
 * stream order).  The query is host only and returns 0 for a shape the entries refuse.
 * Refused (YOND_EINVAL, nothing launched): a null pointer, C % 32 != 0, C outside 32..128, M < 2, a tensor / stat pointer (and, for
 * bwd_apply, dgamma / dbeta) not 16-byte aligned, ws misaligned or smaller than the query's answer, eps < 0 or momentum outside [0, 1]. */
size_t yond_bn_train_ws_bytes(size_t M, int C);
int yond_bn_stats_f32(const float* y, size_t M, int C, const float* gamma, const float* beta, const float* running_mean,
                      const float* running_var, double eps, double momentum, float* stat, float* pending, void* ws, size_t ws_bytes,
                      void* stream);
int yond_bn_apply_relu_f32(const float* y, const float* stat, size_t M, int C, float* out, void* stream);
int yond_bn_bwd_reduce_f32(const float* y, const float* dout, const float* stat, size_t M, int C, float* dgamma, float* dbeta, void* ws,
                           size_t ws_bytes, void* stream);
int yond_bn_bwd_apply_f32(const float* y, const float* dout, const float* stat, const float* dgamma, const float* dbeta, size_t M, int C,
                          float* dy, void* stream);

/* Measurement aid (bench.py; not on the reference's path): one wave sleeps for `us` microseconds (<= 5 s) of wall time and
 * writes out[0] = elapsed shader cycles (s_memtime), out[1] = elapsed 100 MHz reference ticks (s_memrealtime): the clock
 * the chip holds under the load running beside it = out[0] / out[1] * 100 MHz. */
int yond_clock_probe(double us, unsigned long long* out /* [2], device */, void* stream);

/* ------------------------------------------------------------------------------------------------
 * I1  sRGB crop -> raw training pair (img2raw.hip; memory bound, 3 or 6 B in + 8 B out per output)
 * Replaces data_process/yond_datasets.py:277-334 and :483-548 (one item of RGB_Img2Raw_Dataset / DIV2K_Img2Raw_Dataset) with
 * data_process/unprocess.py:80-148 (inverse_smoothstep, gamma_expansion, apply_ccm, safe_invert_gains, clamp, mosaic) and
 * yond_datasets.py:15-19 (bayer_aug), for B crops of one shape in one launch.
 *   crops      uint8 (dtype 0) or uint16 (dtype 1) [..][H][W][3] sRGB crops (device); crop b starts at element patches[b].offset
 *              and needs offset + H*W*3 <= crops_len (a patch outside is written as NaN, nothing is read)
 *   curve      float32 [256] (uint8) or [65536] (uint16) (device): the per-level transfer curve, gamma_expansion(inverse_smoothstep(
 *              level / divisor)) evaluated by the host in the reference's float32 steps (uint8 curves go through LDS)
 *   patches    YondImg2RawPatch [B] (device), one per crop
 *   pattern    0..3: the Bayer rotation of every patch; -1: each patch's own `pattern` (mod 4), only for H == W
 *   hr, lr     float32 [B][4][h'][w'], h' = H/2, w' = W/2 for an even rotation, swapped for an odd one; sigma (optional) float32 [B]
 * Every output element is one pixel of the crop: rotated-mosaic site -> source pixel (Y, X) and channel (Y&1) + (X&1); its three
 * channels go through the curve, out[c] = sum_j in[j] * rgb2cam[c][j], gray = (out0 + out1 + out2) / 3, mask = (max(gray - 0.9, 0)
 * / 0.1)^2, one channel times max(mask + (1 - mask) * g, g), clamped to [0, 1] (float32; the 3-term CCM sums may differ from
 * torch's BLAS in the last bit).  lr = hr + sigma * N(0, 1): Philox4x32-10 keyed by (key, slot), counter = the index of the
 * 4-element group in the patch, Box-Muller -- a patch's noise depends on its key and slot only.  clip != 0 clamps lr to [0, 1].
 * Refused (YOND_EINVAL, nothing launched): a null pointer, H or W odd or < 2, B < 1, a dtype other than 0 / 1, a pattern outside
 * -1..3, pattern -1 with H != W. */
typedef struct {
    float rgb2cam[9];     /* row-major [c][j] (unprocess.py:7-47) */
    float gain[3];        /* [1/red, 1, 1/blue] / rgb_gain in float32 (unprocess.py:112) */
    float sigma;          /* noise standard deviation (already / 255) */
    int pattern;          /* quarter turns of the mosaic (pattern -1 launches) */
    unsigned key, slot;   /* noise stream */
    long long offset;     /* first element of the crop in `crops` */
} YondImg2RawPatch;       /* 72 bytes */
int yond_img2raw_f32(const void* crops, size_t crops_len, int dtype, int H, int W, const float* curve, const YondImg2RawPatch* patches,
                     int B, int pattern, int clip, float* hr, float* lr, float* sigma, void* stream);

/* ------------------------------------------------------------------------------------------------
 * I2  Poisson-Gaussian noise on clean raw data (pgnoise.hip; 4 B in + 4 B out per element)
 * The method's noise model, noisy = Poisson(x / beta1) * beta1 + N(0, beta2) (data_process/yond_datasets.py:720), for B items of
 * n_per_item elements in one launch.  For item b and element i, x = clean[b * n + i], e = exposure, lambda = max(x, 0) * e / beta1:
 *     noisy = (k * beta1) / e + min(x, 0) + sigma_n * z / e,     k ~ Poisson(lambda), z ~ N(0, 1) independent
 * then clamped to [0, 1] when clip is 1.  e = 1, beta1 = K / scale, sigma_n = sigma / scale is the reference's training noise;
 * e = 1 / ratio is a low-light exposure scaled back by ratio.
 *   items      YondPGItem [B] (device); exposure must be finite and > 0, sigma_n finite and >= 0, beta1 finite
 *   clean, noisy  float32 [B][n_per_item] (device), 4-byte aligned (views into tensors are fine), any n_per_item >= 1; either
 *              disjoint or the same pointer (in place)
 * Edges:  beta1 <= 0: no shot noise, noisy = x + sigma_n * z / e.  sigma_n == 0: no read noise, (noisy - min(x, 0)) * e / beta1 is
 * an integer up to one rounding.  x < 0: noisy = x + read noise only (black-level-subtracted ground truth goes slightly negative).
 * x NaN or +-inf: NaN; no other input gives a NaN or an infinity (where x * e / beta1 overflows float32 the shot term is x itself).
 * Sampler (csrc/pgnoise_sampler.h): counter based -- Philox4x32-10 keyed by (key, slot), counter = (64-bit element index, draw
 * number, a tag) -- so noisy[b][i] is a function of (items[b], i, clean[b][i]) alone: not of B, n_per_item, the launch geometry,
 * neighbouring elements or the pointers' alignment.  k is exact in distribution, to the resolution of a 24-bit uniform and float32
 * rounding of the acceptance test (~1e-6), for 0 <= lambda <= 2^23: inversion below lambda = 10 (at most 64 steps), the transformed
 * rejection method PTRS (Hoermann 1993) from 10 to 2^23 (at most 64 attempts, then the normal value).  Above 2^23, where float32 no
 * longer holds every count, k = max(0, rint(lambda + sqrt(lambda) * z')) with a second normal z'.  z is Box-Muller, |z| <= 5.77.
 * Every loop has a fixed bound.  Refused (YOND_EINVAL, nothing launched): a null pointer, a pointer not 4-byte aligned, B < 1 or
 * B > 65535, n_per_item == 0, clip outside {0, 1}. */
typedef struct {
    float beta1;          /* K / scale: the value of one count */
    float sigma_n;        /* read-noise standard deviation, sigma / scale */
    float exposure;       /* e */
    uint32_t key, slot;   /* noise stream */
} YondPGItem;             /* 20 bytes */
int yond_pg_noise_f32(const float* clean, float* noisy, size_t n_per_item, int B, const YondPGItem* items /* device, [B] */, int clip,
                      void* stream);

/* ------------------------------------------------------------------------------------------------
 * I3  Camera noise on clean raw data (camnoise.hip; 4 B in + 4 B out per element, bound by the sampler's arithmetic)
 * The low-light sensor model of data_process/process.py:631-671 (generate_noisy_obs, noise codes p g r q d): what a sensor adds to
 * Poisson-Gaussian noise at exposure ratios of 100-300 -- heavy-tailed (Tukey-lambda) read noise, row noise, quantisation noise and a
 * per-channel dark bias -- for B items of n_per_item elements in one launch.  For item b and element i, x = clean[b * n + i],
 * e = exposure, m = mfm, y = max(x, 0) * e:
 *     shot   Poisson (flag bit 0):     k * beta1 / m,  k ~ Poisson(m * y / beta1)
 *            Gaussian approximation:   y + z_s * sqrt(max(y / beta1, 1e-10)) * beta1 / m           (process.py:646-648)
 *     read   Tukey-lambda (bit 1):     (sig_read / m) * T,  T ~ Tukey-lambda(lam) of scale 1 (sig_read is the SCALE, not the deviation)
 *            Gaussian:                 (sig_read / m) * z
 *     row    (sig_row / m) * z_row, one z_row per row
 *     q      q_step * u_q, u_q uniform on (-0.5, 0.5); NOT divided by m, as in the reference
 *     bias   bias[c], c the element's CFA channel
 *     noisy = clip(shot + read + row + q + bias + min(x, 0) * e) / e,  clip to [clip_lo, clip_hi] when flag bit 2 is set, else none:
 * the clip stands BEFORE the division by e, as process.py:667-669 has it.  (The kernel divides each term by e and clips to
 * [clip_lo / e, clip_hi / e]: the same set of values, and the order of yond_pg_noise_f32's sum.)
 * Degenerate case: flags = Poisson (| clip), sig_row = q_step = 0, bias 0, mfm = 1 gives yond_pg_noise_f32's output BIT FOR BIT for
 * the same (beta1, sig_read, exposure, key, slot) -- with the clip off, and with clip [0, 1] where e = 1.
 * Geometry (what "row" and "channel" mean):
 *   layout 0   packed planar [4][h][row_len]: row = i / row_len (rows of different channels are independent, the reference's (c, h, 1)
 *              draw), channel = i / (n_per_item / 4)
 *   layout 1   Bayer [H][row_len]: row = the sensor row i / row_len, channel = 2 * (row & 1) + (col & 1), as yond_bayer2rggb_f32
 *   row_len 0  no geometry: the caller states that no item has row noise or a bias (yond_public_amd/camnoise.py checks its items; the
 *              items live on the device, this entry point cannot).  An item that has them all the same is ONE row of channel 0.
 *   items      YondCamItem [B] (device); exposure and mfm finite and > 0, sig_* and q_step finite and >= 0, lam finite and > -0.5,
 *              beta1, bias and the clip bounds finite
 *   clean, noisy  float32 [B][n_per_item] (device), 4-byte aligned, any n_per_item >= 1 the geometry divides; disjoint or the same
 *              pointer (in place)
 * Edges:  beta1 <= 0: no shot noise, the shot term is y.  x < 0 carries through: noisy = x + (the other terms) / e.  x NaN or
 * +-inf: NaN; no other input gives a NaN or an infinity.
 * Sampler (csrc/camnoise_sampler.h): counter based on Philox4x32-10 keyed by (key, slot).  k and z are pg_draw's of
 * csrc/pgnoise_sampler.h, same counter and tag; T, u_q and z_s come from one draw under a second tag, counted by the element index;
 * z_row from a third tag with the ROW index in the counter: a function of (key, slot, row) alone.  So noisy[b][i] is a function of
 * (items[b], i, clean[b][i], layout, row_len, n_per_item) and not of B, the launch geometry, neighbours or alignment.
 * T = -+Q_lam(u), Q_lam(u) = (u^lam - (1 - u)^lam) / lam (scipy.stats.tukeylambda.ppf), u uniform on [2^-33, 1/2] with 32 bits and a
 * sign bit: the tail is truncated at |T| <= |Q_lam(2^-33)| -- 1468 at lam = -0.26, 22.9 at lam = 0, 8.85 at lam = 0.102 -- cutting
 * off a mass of 2^-32.  z, z_s, z_row are Box-Muller, |z| <= 5.77.  Every loop has a fixed bound.
 * Refused (YOND_EINVAL, nothing launched): a null pointer, a pointer not 4-byte aligned, B < 1 or B > 65535, n_per_item == 0, a
 * layout outside {0, 1}, row_len < 0, and a row_len > 0 that does not divide the plane n_per_item / 4 (layout 0; n_per_item must
 * then be a multiple of 4) or n_per_item (layout 1), or that comes with n_per_item >= 2^32 (rows and columns are 32-bit). */
#define YOND_CAM_POISSON 1u   /* flags bit 0: Poisson shot noise (else the Gaussian approximation) */
#define YOND_CAM_TUKEY 2u     /* flags bit 1: Tukey-lambda read noise (else Gaussian) */
#define YOND_CAM_CLIP 4u      /* flags bit 2: clip to [clip_lo, clip_hi] before the division by the exposure */
typedef struct {
    float beta1;            /* K / scale */
    float sig_read;         /* Gaussian std, or Tukey-lambda SCALE (not std), / scale */
    float lam;              /* Tukey-lambda shape */
    float sig_row;          /* / scale */
    float q_step;           /* width of the uniform quantisation noise / scale: 1 / scale is the reference's +-0.5 DN; 0 = off */
    float bias[4];          /* per CFA channel, / scale */
    float exposure;         /* e = 1 / ratio */
    float mfm;              /* sqrt(MultiFrameMean) */
    float clip_lo, clip_hi;
    uint32_t flags;         /* YOND_CAM_* */
    uint32_t key, slot;     /* noise stream */
} YondCamItem;              /* 64 bytes */
int yond_camera_noise_f32(const float* clean, float* noisy, size_t n_per_item, int B, const YondCamItem* items /* device, [B] */,
                          int layout, int row_len, void* stream);

/* ------------------------------------------------------------------------------------------------
 * E1 / E2 edge layers of the noise-estimation network EstUnet (estnet.hip; archs/Unet.py:474-611, archs/comp.py:35-126).  The
 * 3x3 layers between them, the pooling and the decoder's transposed 2x2 layers run on yond_conv2d_f32 / yond_maxpool2_f32.
 *   yond_est_conv_in_f32  3x3 on ONE full-resolution plane x [N][H][W], zero padding 1, + bias, ReLU -> dst [N][H][W][Cout].
 *                         w [Cout][9] and bias [Cout] on the device, zero-padded to Cout (a multiple of 32, <= 1024).
 *                         64-bit element offsets.  HBM bound: 4 B in, 4 Cout B out per pixel.
 *   yond_est_head_f32     1x1 from feat [N][H][W][Cin] (Cin a multiple of 4, <= 4096, and out_nc * Cin * 4 + 512 bytes of LDS at most
 *                         64 KiB: Cin = 4096 with out_nc = 4 is YOND_EUNSUPPORTED) to out_nc <= 4 channels (w [out_nc][Cin], bias [out_nc]),
 *                         squared when sq != 0 ('var').  pge 0: out is the map [N][out_nc][H][W].  pge 1: out is the spatial mean
 *                         [N][out_nc]; partial (device, yond_est_head_ws_bytes(N, out_nc) bytes = N * YOND_EST_HEAD_BLOCKS * out_nc
 *                         doubles) holds per-workgroup float64 sums, added in a fixed order by a second launch: the same input gives
 *                         the same bits, no atomics. */
#define YOND_EST_HEAD_BLOCKS 512
int yond_est_conv_in_f32(const float* x, int N, int H, int W, int Cout, const float* w, const float* bias, float* dst, void* stream);
int yond_est_head_f32(const float* feat, int N, int H, int W, int Cin, const float* w, const float* bias, int out_nc, int sq, int pge,
                      float* out, double* partial, void* stream);
size_t yond_est_head_ws_bytes(int N, int out_nc);

/* ------------------------------------------------------------------------------------------------
 * R2 / R3  raw DN <-> the [0, 1] scale, the two ends of a full-frame run (rawio.hip; memory bound: 2 + 4, 4 + 4 and 4 + 2 B per pixel).
 * Replaces the host normalisation of the full-frame datasets (data_process/yond_datasets.py:959-961, 1055-1056:
 * (raw.astype(float32) - bl) * ratio / (wp - bl)) and writes a result back as integer DN.  Flat over n = H * W elements (a stack
 * of frames is one call); pointers need only element alignment, n need not divide by anything.
 *   yond_raw_ingest_u16 / _f32   out[i] = ((float)raw[i] - bl) * ratio / scale, then, with clip01 != 0, x < 0 ? 0 : (x > 1 ? 1 : x).
 *       Three float32 operations, each rounded: subtract, multiply, IEEE divide (no reciprocal, no folded constant) -- bit-equal to
 *       NumPy's evaluation with bl = float32(bl), ratio = float32(ratio), scale = float32(wp - bl) (the difference formed in
 *       double), which is how NumPy takes the Python scalars.  A NaN stays a NaN through the clip, as through np.clip.
 *   yond_raw_emit_u16            y = x[i] * scale; undo_gain != 0: y = y / ratio; y = y + bl; out[i] = (uint16) rint(min(max(y, 0),
 *       65535)).  Every operation rounded on its own (no FMA), ties to even, NaN -> 0.  n_saturated (optional, device): ONE counter
 *       to which the launch ADDS the number of elements whose y was NaN, < 0 or > 65535 (the caller zeroes it when it wants a
 *       per-launch count).  emit(ingest(v), undo_gain) == v for every uint16 v <= wp (tests/test_rawio_host.py).
 * Refused (YOND_EINVAL, nothing launched): a null raw / x / out, n == 0, a pointer that is not aligned to its element. */
int yond_raw_ingest_u16(const uint16_t* raw, size_t n, float bl, float ratio, float scale, int clip01, float* out, void* stream);
int yond_raw_ingest_f32(const float* raw, size_t n, float bl, float ratio, float scale, int clip01, float* out, void* stream);
int yond_raw_emit_u16(const float* x, size_t n, float bl, float scale, float ratio, int undo_gain, uint16_t* out,
                      unsigned long long* n_saturated, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K7r  the robust noise-level fit: utils/isp_algos.py:345-362 with ransac=True (ransac.hip) -- sklearn's RANSACRegressor around a
 * LinearRegression with min_samples = int(sqrt(n)), which the reference ships unused for its host cost (YOND_SIDD.py:85, 113).
 * Every sum is accumulated in a fixed order (no float64 atomics): the same input gives the same bits.
 *   yond_ransac_compact_f32  the pairs (x = mean, y = var) of the elements with lap < *th (th: one float64 on the device; lap may be
 *       null: every element), in the order of NumPy's var[img_lap < th] on the reference's [h][w][nch] arrays: the maps here are
 *       planar [nch][npix] (nch 1..4; flat arrays: nch = 1), the output ascends in pixel * nch + c.  tile_w > 0 (rows of 32 tile_w
 *       pixels): the SIDD_256 re-tiling of YOND_SIDD.py:65, 92-93, whose array is [h][tile_w][32 * nch] -- the output ascends in
 *       ((row * tile_w + j) * 32 + tile) * nch + c for the pixel at column tile * tile_w + j.  polyfit's non-saturation rule
 *       (:348-350) is applied: only 1e-4 < x < 0.8 when that keeps more than 1 % of the selected points, else all of them.
 *       x, y: room for nch * npix floats each.  result (device, 3 int64): {n kept, n selected before the rule, rule applied}.
 *       ws: yond_ransac_compact_ws_bytes(npix) bytes, 8-byte aligned.  Per-workgroup counts (tiles of YOND_RANSAC_TILE pixels),
 *       one scan, one scatter.
 *   yond_ransac_absdev_f32   d[i] = |y[i] - med| in float32, med = (med2[0] + med2[1]) / 2 in float32: np.median's value from the two
 *       middle order statistics (ranks (n - 1) / 2 and n / 2 of yond_select_ranks_f32; device).  sklearn's default
 *       residual_threshold is the median of d.
 *   yond_ransac_trials_f32   idx: int32 [T][m] sample indices into (x, y) (device; T <= YOND_RANSAC_MAXT, 1 <= m <= n); thr2: the two
 *       middle order statistics of d (device).  out (device, [T][YOND_RANSAC_COLS] float64), per trial:
 *         [0] slope, [1] intercept of the centred least-squares line through the trial's samples (float64);
 *         [2] count, [3] Sx, [4] Sy, [5] Sxx, [6] Sxy, [7] Syy, [8] Srr over the inliers, r = |y - (slope x + intercept)| <= thr
 *             in float64 (what sklearn's R^2 and the refit of the winner need);
 *         [9] thr (the float32 threshold, the same in every row).
 *       ws: yond_ransac_ws_bytes(n, T) bytes (per-workgroup partial sums, chunks of YOND_RANSAC_CHUNK points), 8-byte aligned.
 * Refused (YOND_EINVAL, nothing launched): a null pointer other than lap, npix == 0, nch outside 1..4, n < 2, T or m out of range,
 * a misaligned workspace. */
#define YOND_RANSAC_TILE 1024
#define YOND_RANSAC_CHUNK 2048
#define YOND_RANSAC_MAXT 128
#define YOND_RANSAC_COLS 10
size_t yond_ransac_compact_ws_bytes(size_t npix);
int yond_ransac_compact_f32(const float* lap, const float* mean, const float* var, size_t npix, int nch, int tile_w,
                            const double* th, float* x, float* y, long long* result, void* ws, void* stream);
int yond_ransac_absdev_f32(const float* y, size_t n, const float* med2, float* d, void* stream);
size_t yond_ransac_ws_bytes(size_t n, int T);
int yond_ransac_trials_f32(const float* x, const float* y, size_t n, const int32_t* idx, int T, int m, const float* thr2,
                           double* out, void* ws, void* stream);

/* ------------------------------------------------------------------------------------------------
 * M2  illuminance correction, the ELD protocol's brightness alignment before PSNR / SSIM (illum.hip; data_process/__init__.py:139-171
 * IlluminanceCorrect.correct): p = clamp(pred, 0, 1), gain = sum(p * source) / sum(p * p) over the elements whose target is not
 * saturated (source != 1.0f exactly: a target above 1 or a NaN target is included), out = gain * p.  Memory bound: 8 B per element
 * read by the sums, 4 B read and 4 B written by the apply.
 *   layout     which of four groups an element i of the flat arrays adds to:
 *              YOND_ILLUM_BAYER    (y & 1) * 2 + (x & 1) with x = i % width, y = i / width; width and n / width even, n < 2^32
 *              YOND_ILLUM_PACKED4  i & 3; n % 4 == 0
 *              YOND_ILLUM_FLAT     group 0; any n > 0 (width is ignored by this layout and by PACKED4)
 *   yond_illum_sums_f32   sums (device, float64 [5][3]): sums[g] = {num = sum p * source, den = sum p * p, count} of group g = 0..3 over
 *       its included elements, sums[4] = (g0 + g1) + (g2 + g3), the frame's.  Every product is exact in float64 and every addition
 *       is made in an order that depends on (n, layout, the pointers' 16-byte alignment) alone: no float64 atomics, per-workgroup
 *       partials in ws (yond_illum_ws_bytes() bytes, 8-byte aligned) added by a second launch of one workgroup; the same call gives
 *       the same bits.  The grid is a function of n alone: P = ceil(ceil(n / 4) / (YOND_ILLUM_BLOCK_ELEMS / 4)) workgroups up to
 *       YOND_ILLUM_MAX_BLOCKS, above it ceil(P / ceil(P / YOND_ILLUM_MAX_BLOCKS)) of them with a stride loop (every workgroup the same
 *       number of passes).  A NaN prediction in an included element makes its group's num and den and the total's NaN (the
 *       clamp keeps a NaN, as torch.clamp does); under a saturated target it is left out.
 *   yond_illum_apply_f32  out[i] = gain * clamp(pred[i], 0, 1): one float32 multiply with gain = (float)(num / den) formed on the
 *       device from sums -- YOND_ILLUM_FRAME: row 4 (the reference's scalar); YOND_ILLUM_CFA: the row of the element's group (an
 *       extension: per-channel black-level error).  clip != 0: then out > 1 ? 1 : out.  A NaN stays a NaN through clamp and clip.
 *       den == 0 or an empty mask gives what IEEE gives for num / den (NaN or inf times p); nothing is special-cased.  out may be pred.
 * 16-byte accesses when both pointers of a launch are 16-byte aligned and, under BAYER, width % 4 == 0; else one element per lane.
 * Refused (YOND_EINVAL, nothing launched): a null pointer, a float pointer not 4-byte aligned, sums or ws not 8-byte aligned, n == 0,
 * an unknown layout or mode, a geometry the layout does not admit. */
#define YOND_ILLUM_BAYER 0
#define YOND_ILLUM_PACKED4 1
#define YOND_ILLUM_FLAT 2
#define YOND_ILLUM_FRAME 0
#define YOND_ILLUM_CFA 1
#define YOND_ILLUM_MAX_BLOCKS 2048      /* the grid's cap */
#define YOND_ILLUM_BLOCK_ELEMS 4096     /* elements a workgroup takes per pass of its stride loop (256 lanes x 4 vectors of 4) */
size_t yond_illum_ws_bytes(void);
int yond_illum_sums_f32(const float* pred, const float* source, size_t n, int width, int layout, double* sums /* device, [5][3] */,
                        void* ws, void* stream);
int yond_illum_apply_f32(const float* pred, size_t n, int width, int layout, const double* sums /* device */, int mode, int clip,
                         float* out /* may alias pred */, void* stream);

/* ------------------------------------------------------------------------------------------------
 * M3  residual histograms for the noise-model KL divergence (noisehist.hip; utils/sidd_utils.py:280-304 get_histogram / cal_kld): how
 * well a noise model explains the noise of a real frame is the KL divergence between the histogram of noisy - clean and the histogram
 * of residuals drawn from the model on the same clean frame.  The kernels count; the finish (66 numbers) is host code
 * (yond_public_amd/noisekld.py).  B Bayer frames [B][H][W], H and W even, H * W < 2^31.  For every pixel (y, x) of frame f:
 *     r     the residual, ONE float32 subtraction: noisy - clean (NumPy's lr - hr on float32 arrays)
 *     c     the CFA position (y & 1) * 2 + (x & 1), the order of yond_bayer2rggb_f32
 *     b     the intensity band: the number of thresholds[0 .. nb - 2] (float32, ascending, device; may be null when nb == 1) that are
 *           <= clean.  A NaN clean value is in band 0.
 *     bin   np.histogram's rule on edges[ne] (float64, ascending, device: the HOST builds them -- the reference's np.arange edges are
 *           not -R + i * bw to the last bit): bin i holds edges[i] <= r < edges[i + 1] compared in float64, the last bin also
 *           r == edges[ne - 1].  r outside the edges, NaN or +-inf is counted in no bin.
 *     counts[f][b][c][bin] += 1;  counts: unsigned 64-bit [B][nb][4][ne - 1] (device), zeroed by the call.
 *   hint_lo, hint_inv   the kernel's first guess is bin floor((r - hint_lo) * hint_inv) + 1, in float32 (edges[1] and 1 / bin width for the
 *           reference's edges); it then walks to the bin the comparisons with the edges give.  Any values, NaN included, give the same
 *           counts: the hint costs or saves comparisons only.
 *   yond_noise_hist_f32     r = noisy - clean: 8 B read per pixel.
 *   yond_pg_noise_hist_f32  r = v - clean with v the float32 value yond_pg_noise_f32 would have stored for (items[f], element index
 *           y * W + x, clean, clip) -- same sampler, same counter -- without storing it: its counts equal, integer for integer, those of
 *           yond_pg_noise_f32 (n_per_item = H * W) followed by yond_noise_hist_f32.
 * The counts are integers: bit-exact whatever the schedule.  16-byte loads when the pointers are 16-byte aligned and W % 4 == 0, else
 * one element per lane.  grid = (min(ceil(H W / YOND_NOISEHIST_BLOCK_ELEMS), cap / B), B), cap = YOND_NOISEHIST_MAX_BLOCKS, for the fused
 * kernel YOND_NOISEHIST_MODEL_MAX_BLOCKS; every workgroup flushes its LDS histogram once, one 64-bit atomic add per non-zero bin.
 * Refused: YOND_EINVAL for a null pointer, a misaligned pointer (4 bytes for floats, 8 for edges and counts), B outside 1..65535, odd or
 * < 2 H or W, H * W >= 2^31, ne < 2, nb < 1, clip outside {0, 1}; YOND_EUNSUPPORTED for ne - 1 > YOND_NOISEHIST_MAX_BINS,
 * nb > YOND_NOISEHIST_MAX_BANDS or 4 * nb * (ne - 1) > 8448 (the workgroup's LDS histogram). */
#define YOND_NOISEHIST_MAX_BINS 256
#define YOND_NOISEHIST_MAX_BANDS 16
#define YOND_NOISEHIST_MAX_BLOCKS 1024    /* the grid's cap, all frames together: yond_noise_hist_f32 */
#define YOND_NOISEHIST_MODEL_MAX_BLOCKS 6144   /* ... yond_pg_noise_hist_f32 */
#define YOND_NOISEHIST_BLOCK_ELEMS 1024   /* pixels a workgroup takes per pass of its stride loop (256 lanes x 4) */
int yond_noise_hist_f32(const float* noisy, const float* clean, int B, int H, int W, const double* edges /* device */, int ne,
                        const float* thresholds /* device */, int nb, double hint_lo, double hint_inv,
                        unsigned long long* counts /* device */, void* stream);
int yond_pg_noise_hist_f32(const float* clean, int B, int H, int W, const YondPGItem* items /* device, [B] */, int clip,
                           const double* edges /* device */, int ne, const float* thresholds /* device */, int nb, double hint_lo,
                           double hint_inv, unsigned long long* counts /* device */, void* stream);

/* ------------------------------------------------------------------------------------------------
 * M4  defective pixels (bpc.hip): the reference's repair on a list of points (utils/isp_ops.py:152-160 repair_bad_pixels) and, as this
 * project's extension, blind detection from the noise model with the repair in the same pass.  The float64 NumPy model
 * tests/bpc_model.py is the specification.  in / out: float32 Bayer mosaics [H][W], H and W even, H * W < 2^31.
 *     nbh(y, x)   the same-colour 3x3 neighbourhood: the nine pixels (cy(y + 2 dy), cx(x + 2 dx)), dy, dx in {-1, 0, 1}; cy clamps to
 *                 [y & 1, H - 2 + (y & 1)], cx likewise -- cv2.medianBlur(plane, 3)'s replicated border on each plane of bayer2rggb.
 *     m(y, x)     the median of nbh(y, x), centre included, of the INPUT frame: a selection, no rounding.
 *   yond_bpc_repair_list_f32     out[r][c] = m(r, c) for the n points (r, c) of `points` (device int32 [n][2]); every other element of out
 *       is left as it is: out holds a copy of in when the call is made (the reference computes the medians before it writes a point, so
 *       neighbouring listed points do not see each other's repair).  A point outside the frame is skipped; duplicates are harmless.
 *       out == in is accepted for n <= 1 only.  n == 0 launches nothing.
 *   yond_bpc_detect_repair_f32   with hi / lo the maximum / minimum of the eight neighbours without the centre c:
 *           hot   iff c > hi and (c - hi)^2 > t^2 * (beta1 * max(hi, 0) + beta2)
 *           cold  iff c < lo and (lo - c)^2 > t^2 * (beta1 * max(lo, 0) + beta2)
 *       evaluated in float64 from the float32 pixels, every difference, product and sum rounded on its own (no FMA), t^2 = t * t formed
 *       on the host.  (beta1, beta2): variance = beta1 * x + beta2 in the frame's units.  out = m where flagged, else c.
 *       counts   device uint32 [2] = {hot, cold}, 8-byte aligned, zeroed by the caller; exact.  A workgroup adds both with one 64-bit
 *                atomic on the pair (hot is the low word).
 *       coords   device int32 [cap][2] or null: (row, col) of flagged pixels in any order; when more than cap are flagged, cap of them.
 *       out == in is refused: a neighbouring workgroup would read repaired values.
 *       A tile of YOND_BPC_TILE_H x YOND_BPC_TILE_W pixels per workgroup, staged in LDS with a two-pixel halo.  16-byte global accesses
 *       when in and out are 16-byte aligned and W % 4 == 0, 8-byte ones when they are 8-byte aligned, else 4-byte: same values.
 * Non-finite pixels fault nothing; what they give is what v_min / v_max / the comparisons give.
 * Refused (YOND_EINVAL, nothing launched): a null in / out / counts (points with n > 0), a misaligned pointer, H or W odd or < 2,
 * H * W >= 2^31, n < 0, cap < 0, the aliasing named above.  YOND_EUNSUPPORTED: H > 65535 * YOND_BPC_TILE_H. */
#define YOND_BPC_TILE_W 128
#define YOND_BPC_TILE_H 32
int yond_bpc_repair_list_f32(const float* in, float* out, int H, int W, const int* points /* device, [n][2] */, int n, void* stream);
int yond_bpc_detect_repair_f32(const float* in, float* out, int H, int W, double beta1, double beta2, double t,
                               unsigned* counts /* device, [2] */, int* coords /* device, [cap][2], or null */, int cap, void* stream);

/* ------------------------------------------------------------------------------------------------
 * M5  row noise / banding (rownoise.hip): the reference's row_denoise (utils/isp_algos.py:319-334) on a device frame.  The float64 NumPy
 * model tests/rownoise_model.py is the specification.  in / out: float32 Bayer mosaics [H][W], H and W even, H * W < 2^31.  Two launches
 * per frame, no host read between them.  With p = y & 1, j = y >> 1, n = H / 2, r = d / 2:
 *   yond_rownoise_sums_f32    sums[y][c] = the float64 sum of in[y][x] over x % 2 == c (every float32 is exact in float64).  One wave
 *       per row at a time, 16-byte loads when `in` is 16-byte aligned and W % 4 == 0, else one element per lane; a lane's partial sums
 *       are combined by a fixed shuffle tree: the order of the additions depends on W and on that alignment alone, no atomics -- the
 *       same call gives the same bits.  Any order of float64 additions is within (W / 2) * 2^-53 * sum |x| of the exact sum.
 *   yond_rownoise_apply_f32   the sequence of means along the rows of one parity,
 *           per = YOND_ROWNOISE_ROW     m_p[j]     = (sums[y][0] + sums[y][1]) / W        one offset per sensor row: the reference
 *           per = YOND_ROWNOISE_PLANE   m_{p,c}[j] = sums[y][c] / (W / 2)                 one per row of a CFA plane: this project's extension
 *       is smoothed by a 1-D bilateral filter of diameter d with a replicated border, jk = clamp(j + k, 0, n - 1), k = -r .. r:
 *           w_k    = exp(-k^2 / (2 sigma_space^2)) * exp(-(m[jk] - m[j])^2 / (2 sigma_color^2))
 *           offset = m[j] - sum_k w_k m[jk] / sum_k w_k, evaluated as sum_k w_k (m[j] - m[jk]) / sum_k w_k
 *       (the same quantity; in this form equal means give exactly 0 and the rounding error scales with the differences, not with the
 *       level), all in float64, and out[y][x] = (float)((double)in[y][x] - offset[y][x & 1]): one subtraction, one rounding.
 *       Containment: a neighbour whose mean is not finite has weight 0; a row whose own mean is not finite has offset 0; where the
 *       offset is 0 the pixel is copied, bit for bit.  offsets (device float64 [H][2], or null) receives every offset[y][c] once; with
 *       YOND_ROWNOISE_ROW both columns are equal.  A wave computes its row's offsets from `sums` (one tap per lane), then streams the
 *       row.  out may be in exactly (every element is read and written by one lane); otherwise the two frames must not overlap.
 * Refused (YOND_EINVAL, nothing launched): a null in / out / sums, a pointer off its element size (sums, offsets: 8 bytes), H or W odd or
 * < 2, H * W >= 2^31, d even or outside [1, YOND_ROWNOISE_MAX_D], sigma_color / sigma_space not finite or <= 0 (or so small that 2 sigma^2 is 0 in float64), an unknown per, an out that overlaps in
 * without being in. */
#define YOND_ROWNOISE_ROW 0
#define YOND_ROWNOISE_PLANE 1
#define YOND_ROWNOISE_MAX_D 63
int yond_rownoise_sums_f32(const float* in, int H, int W, double* sums /* device, [H][2] */, void* stream);
int yond_rownoise_apply_f32(const float* in, float* out, int H, int W, const double* sums /* device, [H][2] */, int per, int d,
                            double sigma_color, double sigma_space, double* offsets /* device, [H][2], or null */, void* stream);

/* ------------------------------------------------------------------------------------------------
 * I4  clean raw frames -> raw training pairs (rawcrop.hip; memory bound, 2 B in + 8 B out per output)
 * Replaces data_process/yond_datasets.py:153-212 (one item of SID_Raw_Dataset: DN normalisation, Bayer-pattern rotation, packing,
 * clip, square-root augmentation, crops, brightness / white-balance jitter, AWGN) for B patches of one side in one call.
 *   frames     uint16 (dtype 0) or float32 DN (dtype 1) [..][H][W] Bayer frames (device), frames_len elements in all; patch b reads
 *              the frame that starts at element patches[b].frame
 *   patches    YondRawCropPatch [B] on the HOST: read and checked before anything is launched, then handed to the kernel by value
 *              (RC_CHUNK = 64 patches per launch; a batch of up to 64 is one launch).  The array is free again when the call returns.
 *   hr, lr     float32 [B][4][ps][ps] (device); sigma float32 [B] (device): sigma[b] = patches[b].sigma
 * Output element hr[b][c][y][x], c = 2 dy + dx (bayer2rggb): the rotated frame is np.rot90(frame, pattern) of (H, W) or (W, H), its
 * packed position (y0 + y, x0 + x) and sub-site (dy, dx) name one source pixel DN.  In float32, every step rounded once:
 *     v = (float(DN) - bl) / (wp - bl)        true subtract and divide
 *     v = min(max(v, 0), 1);  v = sqrt(v) if vst_aug;  v = v * rgb_gain
 *     c == 0: v = float(double(v) * gain0);   c == 2: v = float(double(v) * gain2)       (the reference's float32 plane times a
 *                                                                                          float64 ratio, stored to float32)
 *     hr = v;  lr = v + z * sigma
 * z is standard normal: Philox4x32-10 keyed by (key, slot), counter = (element index in the patch) / 4, Box-Muller; element
 * index % 4 picks one of the call's four normals.  lr[b] is a function of (patches[b], element) alone.  clip != 0 clamps hr and lr
 * to [0, 1].  DN must be finite.  16-byte stores when hr and lr are 16-byte aligned, 4-byte stores otherwise: same values.
 * Refused (YOND_EINVAL, nothing launched, nothing written): a null pointer, H or W odd or < 2, B < 1, ps < 1 or > 16384, a dtype other
 * than 0 / 1, wp <= bl, and for any patch a pattern outside 0..3, a vst_aug outside {0, 1}, a crop that leaves the rotated frame
 * (y0 < 0, x0 < 0, y0 + ps > h', x0 + ps > w'), frame < 0 or frame + H * W > frames_len. */
typedef struct {
    long long frame;        /* first element of the Bayer frame in `frames` */
    int y0, x0;             /* crop origin in PACKED coordinates of the ROTATED frame */
    int pattern;            /* k of np.rot90(bayer, k, axes=(-2,-1)), 0..3 */
    int vst_aug;            /* 1: hr = sqrt(hr) after the [0,1] clip */
    float rgb_gain;         /* 1 when the item draws no gains */
    double gain0, gain2;    /* multipliers of packed channels 0 and 2; 1 when none */
    float sigma;
    unsigned key, slot;     /* noise stream */
} YondRawCropPatch;         /* 64 bytes */
int yond_rawcrop_f32(const void* frames, size_t frames_len, int dtype /*0 u16, 1 f32*/, int H, int W, float bl, float wp,
                     const YondRawCropPatch* patches, int B, int ps /* packed patch side */, int clip, float* hr, float* lr,
                     float* sigma, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* YOND_HIP_H */
