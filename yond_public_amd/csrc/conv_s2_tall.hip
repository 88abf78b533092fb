// S2t: the 3x3 stride-2 layer at split precision on 8-ROW tiles, two output rows per wave (descriptor algo 7), in two forms: ONE input image
// in LDS with the weights beside it, or TWO input images with the weights in registers (yond_conv_s2_tall_dispatch chooses per depth).
//
// The same arithmetic as the stride-2 form of conv_split_kernel.h (its header: split operands, three v_mfma_f32_32x32x16_f16 per fp32 product,
// two accumulators) and, per accumulator, the same MFMA sequence -- chunk order, tap order (dx outermost, dy inside), h_w l_x, then h_w h_x, then
// l_w h_x -- and the operations of its epilogue_direct (with the second output's loop) in their order: bit-identical results.  Another tile:
//   * 8 output rows x 32 pixels x 64 channels per persistent 512-thread workgroup; waves = 4 row groups x 2 channel blocks, a wave owns TWO
//     output rows x 32 channels (2 x 2 accumulators).  It reads input rows 0..4 of its group: the middle row's fragments serve both output
//     rows and every weight fragment serves both -- 30 pixel + 18 weight fragments for 54 MFMAs per 16-channel step where the 4-row tile reads
//     18 + 18 for 27, and the step's fixed cost (head, barrier wait, tail, the first fragments behind the barrier) is paid once per 54;
//   * the input image of a chunk: 17 rows in the template's stride-2 layout (planes [channel half][part][17 x 66 units], even and odd columns in
//     separate halves of a row, the zero unit for pixels outside the frame) = 71.8 KB.
// ONE IMAGE (conv_s2_tall_kernel_one_image): the image, two weight buffers of 36.9 KB filled by LDS-DMA one step ahead, the scale / shift
// vectors; two images do not fit beside the weights.  A step is: MFMAs on image(s) and weights(s), between them the global loads of chunk
// s+1's units into ONE register set (9 x 16 bytes per thread) and the weight DMA of s+1 | barrier: every wave is done reading the image |
// ds_write_b128 of the held units | barrier.  Nothing covers that write phase.
// TWO IMAGES (conv_s2_tall_kernel): the weights never enter LDS -- a 16-byte unit of the packed layout is a lane's A fragment, so a wave
// loads the 18 fragments of its own 32-channel block from global memory (the four row-group waves of a block read the same bytes: the CU's
// vector cache serves most of it) -- and two images fit: 2 x 73.7 KB + the vectors = 156 KB.  Step s multiplies image(s & 1) while LDS-DMA
// with per-lane source addresses fills image((s + 1) & 1): no register set, no ds_write, ONE barrier per step.  ONE set of weight registers
// (two sets and the accumulators exceed a wave's 256 registers at two waves per SIMD): a tap row of chunk s+1 is loaded into its registers
// right behind its last use in step s.
// In both forms a tile's first chunk is requested during the previous tile's last step, ahead of its epilogue.
// The packed weights are what yond_pack_conv_split_weight_f32 writes for the template ([channel tile][chunk][tap][channel half][part][64][8]).
// Covered: split planes in, planes of 4 channels out, tn 64, bias or (per-image) scale + shift, no activation or LeakyReLU, with and without
// the second output (SiLU(value) in split planes: a producer of halves, it raises YOND_STATUS_HALF_OVERFLOW where the template does).
// Everything else stays on the template (yond_conv_s2_tall_supported).
#include "common.h"

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
#define S2T_GLOBAL __attribute__((address_space(1)))

namespace {
constexpr int S2T_TH = 8;                                   // output rows of a tile
constexpr int S2T_IH = (S2T_TH - 1) * 2 + 3;                // 17 input rows
constexpr int S2T_IW = 31 * 2 + 3;                          // 65 input columns
constexpr int S2T_HALF = (S2T_IW + 1) / 2;                  // even columns | odd columns
constexpr int S2T_TWP = 2 * S2T_HALF;                       // units of an LDS row
constexpr int S2T_PLANE = S2T_IH * S2T_TWP * 4;             // floats of a plane's LDS image
constexpr int S2T_IMG = 4 * S2T_PLANE + 4;                  // four planes [channel half][part]; the last unit takes the items past the tile
constexpr int S2T_W = 9 * 2 * 2 * 64 * 4;                   // floats of a weight slice [tap][channel half][part][64] x 16 bytes
constexpr int S2T_NWV = S2T_W / 4;                          // its 16-byte units
constexpr int S2T_NWT = (S2T_NWV + 511) / 512;              // LDS-DMA instructions per thread and step (the last one: waves 0..3)
constexpr int S2T_NITEM = S2T_IH * S2T_IW * 4;              // 16-byte units of a chunk's image: pixel x plane
constexpr int S2T_NIN = (S2T_NITEM + 511) / 512;            // ... per thread: the register set
constexpr int S2T_FILM = 1536;                              // floats: scale[images x Cout], then shift -- of every image and channel tile, copied once
constexpr int S2T_W_OFF = S2T_IMG, S2T_FILM_OFF = S2T_W_OFF + 2 * S2T_W;
constexpr int S2T_SMEM = (S2T_FILM_OFF + 2 * S2T_FILM) * 4;
static_assert(S2T_SMEM <= 160 * 1024, "LDS budget");
static_assert((S2T_NIN - 1) * 512 < S2T_NITEM, "only a thread's last item may lie past the tile");
// The two-image form: an image is S2T2_NDMA x 8 wave-instructions of 64 units -- the four planes and, behind them, units that
// only ever receive the zero unit, so that every wave issues the same number of whole instructions and none writes past its image.
constexpr int S2T2_NDMA = (4 * S2T_IH * S2T_TWP + 511) / 512;  // LDS-DMA instructions per thread and step
constexpr int S2T2_IMG = S2T2_NDMA * 512 * 4;                // floats of an image
constexpr int S2T2_FILM_OFF = 2 * S2T2_IMG;
constexpr int S2T2_SMEM = (S2T2_FILM_OFF + 2 * S2T_FILM) * 4;
static_assert(S2T2_SMEM <= 160 * 1024, "LDS budget");
static_assert(S2T2_NDMA == S2T_NIN, "both forms keep one offset per thread and instruction");
__device__ __forceinline__ float s2t_silu(float x) {        // (conv_split_kernel.h, split_silu)
    return x * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(x * -1.44269504088896341f));
}
}  // namespace

// TWO = false: the one-image form of the header.  TWO = true: the two-image form (the comment ahead of its step, below).
template <bool D2, bool TWO>
__device__ __forceinline__ void s2t_body(const YondConvDesc& d) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int FILM_OFF = TWO ? S2T2_FILM_OFF : S2T_FILM_OFF;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, lh = lane >> 5;
    const int rg = wave & 3, cg = wave >> 2;                 // row group (output rows 2 rg, 2 rg + 1), 32-channel block
    const int nct = d.Cout / 64, ntx = (d.Wo + 31) / 32, nty = (d.Ho + S2T_TH - 1) / S2T_TH;
    const int total = nct * ntx * nty * d.N;
    const int G = gridDim.x;
    // (the template's walk: tile index digits (n, ty, tx, ct), workgroups of one XCD take contiguous runs -- the sibling channel tiles share an L2)
    const int lslot = (G % 8 == 0) ? (blockIdx.x % 8) * (G / 8) + blockIdx.x / 8 : blockIdx.x;
    const int nchunk = d.C0 / 16;
    const bool rev = d.tile_order != 0;                      // (the spatial digits complemented: results do not depend on it)
    const int PS0 = YOND_SP_PLANE_UNITS(d.H, d.W);
    if (lslot >= total) return;
    const bool clk_on = d.clk != nullptr && blockIdx.x == 0 && tid == 0;       // measurement aid (YondConvDesc.clk)
    unsigned long long clk_c0 = 0, clk_r0 = 0;
    if (clk_on) { clk_c0 = __builtin_amdgcn_s_memtime(); clk_r0 = __builtin_amdgcn_s_memrealtime(); }
    // (values that live through the whole kernel and are needed once per tile or once per launch wait in vector registers: the scalar file is full)
    asm volatile("" : "+v"(clk_c0), "+v"(clk_r0));
    float* dst_v = d.dst;
    char* dst2_v = (char*)d.dst2;
    unsigned int* word_v = d.status;
    unsigned long long* clk_v = d.clk;
    asm volatile("" : "+v"(dst_v), "+v"(dst2_v), "+v"(word_v), "+v"(clk_v));
    int nct_v = nct, ntx_v = ntx, nty_v = nty;               // (the tile index's digits: a few divisions once per tile)
    unsigned ps2_v = (unsigned)YOND_SP_PLANE_UNITS(d.Ho, d.Wo);
    asm volatile("" : "+v"(nct_v), "+v"(ntx_v), "+v"(nty_v), "+v"(ps2_v));

    // the scale / shift vectors of every image and channel, once (visible behind the prologue's barrier)
    {
        const int nf = (d.ebatch ? d.N : 1) * d.Cout;
        for (int i = tid; i < nf; i += 512) {
            smem[FILM_OFF + i] = d.escale ? d.escale[i] : 1.0f;
            smem[FILM_OFF + S2T_FILM + i] = d.eshift ? d.eshift[i] : 0.0f;
        }
    }

    // one image: the thread's items: it = tid + 512 k -> plane it & 3 (channel half x part), pixel it >> 2 of the 17 x 65 image
    int in_lds[TWO ? 1 : S2T_NIN];
    if constexpr (!TWO) {
#pragma unroll
        for (int k = 0; k < S2T_NIN; ++k) {
            const int it = tid + k * 512;
            const int pix = it >> 2, py = pix / S2T_IW, px = pix % S2T_IW;
            const int lp = py * S2T_TWP + (px & 1) * S2T_HALF + (px >> 1);
            in_lds[k] = it < S2T_NITEM ? (it & 3) * S2T_PLANE + lp * 4 : 4 * S2T_PLANE;
        }
    }

    struct Tile { int ct, n, ox0, oy0; };
    auto origin = [&](int t) {
        Tile T;
        int b = t;
        T.ct = b % nct_v; b /= nct_v;
        const int tx = b % ntx_v; b /= ntx_v;
        const int ty = b % nty_v, n = b / nty_v;
        T.n = __builtin_amdgcn_readfirstlane(rev ? d.N - 1 - n : n);
        T.ct = __builtin_amdgcn_readfirstlane(T.ct);
        T.ox0 = __builtin_amdgcn_readfirstlane((rev ? ntx_v - 1 - tx : tx) * 32);
        T.oy0 = __builtin_amdgcn_readfirstlane((rev ? nty_v - 1 - ty : ty) * S2T_TH);
        return T;
    };
    // byte offsets of the thread's units from the chunk's first plane: the zero unit behind the plane for a pixel outside the image
    // (the dispatcher keeps a chunk's four planes below 2^31 bytes)
    unsigned voff[S2T_NIN];
    auto decode = [&](const Tile& T) {
#pragma unroll
        for (int k = 0; k < S2T_NIN; ++k) {
            if constexpr (TWO) {
                // lane l of wave-instruction 8 k + wave owns LDS unit u = tid + 512 k of the image: the pixel is derived from the unit.  The
                // layout's pad units (column 65 of a row) and the units behind the four planes take the zero unit as well
                const int u = tid + k * 512;
                const int pl = u / (S2T_IH * S2T_TWP), rem = u - pl * (S2T_IH * S2T_TWP);
                const int py = rem / S2T_TWP, c = rem - py * S2T_TWP, hf = c >= S2T_HALF ? 1 : 0, px = 2 * (c - hf * S2T_HALF) + hf;
                const int gy = T.oy0 * 2 - 1 + py, gx = T.ox0 * 2 - 1 + px;
                const bool in = pl < 4 && px < S2T_IW && gy >= 0 && gy < d.H && gx >= 0 && gx < d.W;
                voff[k] = ((unsigned)(pl & 3) * (unsigned)PS0 + (unsigned)(in ? gy * d.W + gx : d.H * d.W)) * 16u;
            } else {
                const int it = tid + k * 512;
                const int pix = it >> 2, py = pix / S2T_IW, px = pix % S2T_IW;
                const int gy = T.oy0 * 2 - 1 + py, gx = T.ox0 * 2 - 1 + px;
                const bool in = it < S2T_NITEM && gy >= 0 && gy < d.H && gx >= 0 && gx < d.W;
                voff[k] = ((unsigned)(it & 3) * (unsigned)PS0 + (unsigned)(in ? gy * d.W + gx : d.H * d.W)) * 16u;
            }
        }
    };
    auto uniform_ptr = [&](const void* p) {                  // wave-uniform: handed to the memory instructions in scalar registers
        const unsigned long long a = (unsigned long long)(uintptr_t)p;
        const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a), hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
        return (const char*)(uintptr_t)(((unsigned long long)hi << 32) | lo);
    };
    // (the units' base stays a pointer derived from the kernel argument -- global loads, not flat ones; uniform: its operands are)
    auto in_base = [&](const Tile& T, int ch) { return (const char*)d.src0 + (size_t)(T.n * nchunk + ch) * 4 * (size_t)PS0 * 16; };
    auto w_base = [&](const Tile& T, int ch) { return uniform_ptr(d.wpk + ((size_t)T.ct * nchunk + ch) * S2T_W); };
    f32x4 vin[TWO ? 1 : S2T_NIN];                             // one image: the ONE register set: chunk s+1's units, held until the image is free
    auto issue_load = [&](auto kc, const char* ib) __attribute__((always_inline)) {
        constexpr int k = decltype(kc)::value;
        vin[k] = *(const S2T_GLOBAL f32x4*)(const S2T_GLOBAL char*)(ib + voff[k]);
    };
    // weight slice global -> LDS by LDS-DMA as inline assembly (conv_split_kernel.h, issue_dma): one instruction moves 512 x 16 bytes
    auto issue_dma = [&](auto kc, const char* wsrc, float* wbuf) __attribute__((always_inline)) {
        constexpr int k = decltype(kc)::value;
        const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) float*)wbuf;
        const int it = tid + k * 512;
        const int it_wave = __builtin_amdgcn_readfirstlane(it - lane);
        const unsigned lds_wave = __builtin_amdgcn_readfirstlane(lds0 + (unsigned)it_wave * 16u);
        const unsigned vo = (unsigned)it * 16u;
        // (only the slice's last, partial pass needs the test: a branch in the middle of the MFMA stretch ends a scheduling region)
        if ((k + 1) * 512 <= S2T_NWV || it_wave < S2T_NWV)
            asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(lds_wave), "v"(vo), "s"(wsrc) : "memory");
    };
    auto write_in = [&]() __attribute__((always_inline)) {
        if constexpr (!TWO) {
#pragma unroll
            for (int k = 0; k < S2T_NIN; ++k) *(f32x4*)(smem + in_lds[k]) = vin[k];
        }
    };
    // two images: the wave's instruction k of an image, global -> LDS with per-lane source addresses (conv_split_kernel.h, issue_in_dma)
    auto issue_in_dma = [&](auto kc, const char* ib, float* img) __attribute__((always_inline)) {
        constexpr int k = decltype(kc)::value;
        const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) float*)img;
        const unsigned lds_wave = __builtin_amdgcn_readfirstlane(lds0 + (unsigned)((k * 8 + wave) * 1024));
        const unsigned vo = voff[k];
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(lds_wave), "v"(vo), "s"(ib) : "memory");
    };
    // two images: the weights never enter LDS.  A 16-byte unit of the packed layout is a lane's A fragment (gemm_k1_stationary.hip relies on
    // the same); the wave's 18 fragments [dx][dy][part] of a chunk, its own 32-channel block.  ONE set (two do not fit 256 registers beside
    // the accumulators): a tap row of chunk s+1 is fetched into its registers right behind its last use in step s (the template's WINPLACE)
    f16x8 wr[3][3][2];
    const unsigned w_goff = (unsigned)((((lane >> 5) * 2) * 64 + (wave >> 2) * 32 + (lane & 31)) * 16);
    auto load_wr = [&](auto dc, auto yc, const char* ws) __attribute__((always_inline)) {
        constexpr int dx = decltype(dc)::value, dy = decltype(yc)::value;
#pragma unroll
        for (int p = 0; p < 2; ++p)
            wr[dx][dy][p] = *(const S2T_GLOBAL f16x8*)(const S2T_GLOBAL char*)(ws + w_goff + (unsigned)((((dy * 3 + dx) * 4 + p) * 64) * 16));
    };

    f32x16 acc[2][2];                                         // [0] h_w h_x ; [1] the two cross terms (carry the 2^11 scale)  x  output row
    auto zero_acc = [&]() {
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[a][m][r] = 0.0f;
    };

    // ---- the multiplications of one step: groups q = (dx, input row r); fragment X(r, dx) serves output row m with tap row dy = r - 2 m ----
    const int x_off = (lh * 2) * S2T_PLANE + ((rg * 4) * S2T_TWP + li) * 4;
    const int w_off = ((lh * 2) * 64 + cg * 32 + li) * 4;
    const bool wave_hi = wave >= 4;
    const char* ib_s = nullptr;
    const char* wsrc_s = nullptr;
    auto mfma_step = [&](const float* wcur, float* wnext, auto&& prep) __attribute__((always_inline)) {
        typedef const __attribute__((address_space(3))) f16x8* lds_h8;
        const __attribute__((address_space(3))) float* xb = (const __attribute__((address_space(3))) float*)(smem + x_off);
        const __attribute__((address_space(3))) float* wb = (const __attribute__((address_space(3))) float*)(wcur + w_off);
        constexpr int R = 5, NQ = 3 * R, XD = 3, Q0 = 2, NQW = NQ - Q0, NOPS = S2T_NWT + S2T_NIN;
        f16x8 xr[XD][2], wt[2][3][2];                         // pixel fragments two groups ahead; the weight fragments of a column, the next column's fetched during it
        auto loadX = [&](auto qc) __attribute__((always_inline)) {
            constexpr int q = decltype(qc)::value, dx = q / R, r = q % R;
            constexpr int xo = (dx & 1) * S2T_HALF + (dx >> 1);
#pragma unroll
            for (int p = 0; p < 2; ++p) xr[q % XD][p] = *(lds_h8)(xb + p * S2T_PLANE + (r * S2T_TWP + xo) * 4);
        };
        auto loadW = [&](auto dc) __attribute__((always_inline)) {
            constexpr int dx = decltype(dc)::value;
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int p = 0; p < 2; ++p) wt[dx % 2][dy][p] = *(lds_h8)(wb + (((dy * 3 + dx) * 4 + p) * 64) * 4);
        };
        loadW(IntC<0>{});
        loadX(IntC<0>{});
        loadX(IntC<1>{});
        static_for<0, NQ>([&](auto qc) __attribute__((always_inline)) {
            constexpr int q = decltype(qc)::value, dx = q / R, r = q % R;
            constexpr bool wpre = r == 2 && dx < 2;
            if constexpr (q + 2 < NQ) loadX(IntC<q + 2>{});
            if constexpr (wpre) loadW(IntC<dx + 1>{});
            constexpr int nmf = 3 * ((r <= 2 ? 1 : 0) + (r >= 2 ? 1 : 0));
#pragma unroll
            for (int a = 0; a < 3; ++a) {                     // 0: h_w l_x   1: h_w h_x   2: l_w h_x
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    const int dy = r - 2 * m;
                    if (dy < 0 || dy > 2) continue;
                    acc[a == 1 ? 0 : 1][m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wt[dx % 2][dy][a == 2 ? 1 : 0], xr[q % XD][a == 0 ? 1 : 0],
                                                                                    acc[a == 1 ? 0 : 1][m], 0, 0, 0);   // D = W . X^T
                }
            }
            // (the older wave of a SIMD wins the issue arbitration: the younger half leads for the first half of the step -- conv_split_kernel.h)
            if constexpr (q == 0) { if (wave_hi) __builtin_amdgcn_s_setprio(1); }
            if constexpr (q == NQ / 2) { if (wave_hi) __builtin_amdgcn_s_setprio(0); }
            if constexpr (q == Q0 - 1) prep();
            // this group's share of the step's vector-memory instructions: the weight DMA of step s+1, then the loads of its units
            constexpr int qq = q >= Q0 ? q - Q0 : 0;
            constexpr int o_lo = q >= Q0 ? (qq * NOPS + NQW - 1) / NQW : 0, o_hi = q >= Q0 ? ((qq + 1) * NOPS + NQW - 1) / NQW : 0;
            static_for<o_lo, (o_hi < NOPS ? o_hi : NOPS)>([&](auto oc) __attribute__((always_inline)) {
                constexpr int o = decltype(oc)::value;
                if constexpr (o < S2T_NWT) issue_dma(IntC<o>{}, wsrc_s, wnext);
                else issue_load(IntC<o - S2T_NWT>{}, ib_s);
            });
            // Issue order of the group: its LDS reads first (two groups / one column ahead of their use), then its MFMAs with the group's unit loads behind the first
            constexpr int nrd = (q + 2 < NQ ? 2 : 0) + (wpre ? 6 : 0);
            constexpr int l_lo = o_lo > S2T_NWT ? o_lo : S2T_NWT, nld = o_hi > l_lo ? o_hi - l_lo : 0;
            if constexpr (nrd > 0) __builtin_amdgcn_sched_group_barrier(0x100, nrd, 0);
#pragma unroll
            for (int i = 0; i < nmf; ++i) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                if (i == 0 && nld > 0) __builtin_amdgcn_sched_group_barrier(0x020, nld, 0);
            }
        });
    };

    // ---- the two-image step: the same groups and MFMAs on image(s) and the weight registers; between them the wave's S2T2_NDMA
    // instructions of image(s+1) (groups Q0 .. QE - 1) and, behind the last reader of a tap row, its two fragments of chunk s+1.
    // Vector-memory operations complete in issue order, so once at most S2T2_AFTER of them are pending -- the fragment loads issued behind
    // the last DMA -- the wave's share of image(s+1) is in LDS: the count the step's one barrier waits for ----
    constexpr int S2T2_QE = 10;
    constexpr int S2T2_AFTER = 2 * (5 - ((S2T2_QE - 1) % 5 > 2 ? (S2T2_QE - 1) % 5 : 2) + 3 * (2 - (S2T2_QE - 1) / 5));   // group QE - 1 and later: rows r >= 2
    static_assert(S2T2_QE > 2 && S2T2_QE <= 15, "the DMAs sit in groups Q0 .. QE - 1");
    auto mfma_step2 = [&](const float* img, float* inext, auto&& prep) __attribute__((always_inline)) {
        typedef const __attribute__((address_space(3))) f16x8* lds_h8;
        const __attribute__((address_space(3))) float* xb = (const __attribute__((address_space(3))) float*)(img + x_off);
        constexpr int R = 5, NQ = 3 * R, XD = 3, Q0 = 2, NQW = S2T2_QE - Q0, NOPS = S2T2_NDMA;
        f16x8 xr[XD][2];                                      // pixel fragments two groups ahead
        auto loadX = [&](auto qc) __attribute__((always_inline)) {
            constexpr int q = decltype(qc)::value, dx = q / R, r = q % R;
            constexpr int xo = (dx & 1) * S2T_HALF + (dx >> 1);
#pragma unroll
            for (int p = 0; p < 2; ++p) xr[q % XD][p] = *(lds_h8)(xb + p * S2T_PLANE + (r * S2T_TWP + xo) * 4);
        };
        loadX(IntC<0>{});
        loadX(IntC<1>{});
        static_for<0, NQ>([&](auto qc) __attribute__((always_inline)) {
            constexpr int q = decltype(qc)::value, dx = q / R, r = q % R;
            constexpr bool wrep = r >= 2;                      // tap row dy = r - 2 has its last use (output row 1) in this group
            if constexpr (q + 2 < NQ) loadX(IntC<q + 2>{});
            constexpr int nmf = 3 * ((r <= 2 ? 1 : 0) + (r >= 2 ? 1 : 0));
#pragma unroll
            for (int a = 0; a < 3; ++a) {                     // 0: h_w l_x   1: h_w h_x   2: l_w h_x
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    const int dy = r - 2 * m;
                    if (dy < 0 || dy > 2) continue;
                    acc[a == 1 ? 0 : 1][m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wr[dx][dy][a == 2 ? 1 : 0], xr[q % XD][a == 0 ? 1 : 0],
                                                                                    acc[a == 1 ? 0 : 1][m], 0, 0, 0);   // D = W . X^T
                }
            }
            if constexpr (q == 0) { if (wave_hi) __builtin_amdgcn_s_setprio(1); }
            if constexpr (q == NQ / 2) { if (wave_hi) __builtin_amdgcn_s_setprio(0); }
            if constexpr (q == Q0 - 1) prep();
            constexpr bool dq = q >= Q0 && q < S2T2_QE;
            constexpr int qq = dq ? q - Q0 : 0;
            constexpr int o_lo = dq ? (qq * NOPS + NQW - 1) / NQW : 0, o_hi = dq ? ((qq + 1) * NOPS + NQW - 1) / NQW : 0;
            static_for<o_lo, (o_hi < NOPS ? o_hi : NOPS)>([&](auto oc) __attribute__((always_inline)) { issue_in_dma(oc, ib_s, inext); });
            if constexpr (wrep) load_wr(IntC<dx>{}, IntC<r - 2>{}, wsrc_s);
            // Issue order of the group: its LDS reads, its MFMAs, then the fragment loads behind their registers' last reader
            if constexpr (q + 2 < NQ) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
#pragma unroll
            for (int i = 0; i < nmf; ++i) __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            if constexpr (wrep) __builtin_amdgcn_sched_group_barrier(0x020, 2, 0);
        });
    };

    // ---- output: lane = pixel, planes of 4 channels -- the operations of the template's epilogue_direct in its order ----
    float slope_eff = d.post_act == 2 ? d.slope : 1.0f;
    asm volatile("" : "+v"(slope_eff));
    YondRange amax;                                           // largest |value| this thread has stored as halves (range guard)
    auto epilogue = [&](const Tile& T) __attribute__((always_inline)) {
        const int ox = T.ox0 + li;
        const bool col_ok = ox < d.Wo;
        const int cbase = T.ct * 64 + cg * 32 + 4 * lh;
        const float* fs = smem + FILM_OFF + (d.ebatch ? T.n * d.Cout : 0) + cbase;
        const long long hw = (long long)d.Ho * d.Wo;
        f32x4 es[4], et[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            es[g] = *(const f32x4*)(fs + 8 * g);
            et[g] = *(const f32x4*)(fs + S2T_FILM + 8 * g);
        }
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const int oy = T.oy0 + rg * 2 + m;
            const bool ok = col_ok && oy < d.Ho;
            const long long pixo = (long long)oy * d.Wo + ox;
            float* op = dst_v + (((long long)T.n * (d.Cout / 4) + cbase / 4) * hw + pixo) * 4;
            const long long gstep = 8LL * hw;                 // elements from one 8-channel group to the next
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f32x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float x = acc[0][m][4 * g + e];
                    x = fmaf(acc[1][m][4 * g + e], 1.0f / 2048.0f, x);
                    x = fmaf(x, es[g][e], et[g][e]);
                    x = x > 0.0f ? x : x * slope_eff;
                    v[e] = x + 0.0f;
                }
                if (ok) *(S2T_GLOBAL f32x4*)(S2T_GLOBAL float*)(op + g * gstep) = v;
                if constexpr (D2) {
                    // second output: SiLU(v) split into (h, l); a lane holds HALF a 16-byte unit (4 of a pixel's 8 consecutive channels)
                    f32x4 a;
#pragma unroll
                    for (int e = 0; e < 4; ++e) a[e] = s2t_silu(v[e]);
                    amax.add(a);
                    const f16x4 h = {(_Float16)a[0], (_Float16)a[1], (_Float16)a[2], (_Float16)a[3]};
                    const int c8 = cbase - 4 * lh + 8 * g;      // first channel of the lane's unit
                    const size_t PS2 = (size_t)ps2_v;
                    char* pp = dst2_v + ((size_t)(((T.n * (d.Cout / 16) + (c8 >> 4)) * 2 + ((c8 >> 3) & 1)) * 2) * PS2 + (size_t)pixo) * 16 + lh * 8;
                    if (ok) *(S2T_GLOBAL f16x4*)(S2T_GLOBAL char*)pp = h;
                    const f16x4 l = {(_Float16)((a[0] - (float)h[0]) * 2048.0f), (_Float16)((a[1] - (float)h[1]) * 2048.0f),
                                     (_Float16)((a[2] - (float)h[2]) * 2048.0f), (_Float16)((a[3] - (float)h[3]) * 2048.0f)};
                    if (ok) *(S2T_GLOBAL f16x4*)(S2T_GLOBAL char*)(pp + PS2 * 16) = l;
                }
            }
        }
    };

    // ---- the step pipeline ----
    struct Cur { int tile, ch; };
    auto adv = [&](Cur c) {
        Cur n;
        const bool last = c.ch + 1 == nchunk;
        n.tile = last ? c.tile + G : c.tile;
        n.ch = last ? 0 : c.ch + 1;
        return n;
    };
    Cur cs = {lslot, 0};
    Tile lt = origin(lslot), cur = lt;                        // tile of the loads / of the accumulators (epilogue)
    auto park = [&](Tile& T) { asm volatile("" : "+v"(T.ct), "+v"(T.n), "+v"(T.ox0), "+v"(T.oy0)); };
    park(cur);
    if constexpr (TWO) {
        // ---- two images: step s multiplies image(s & 1) while image((s + 1) & 1) is filled; ONE barrier per step.  The image being filled
        // was last read in step s - 1, and every wave has passed that step's barrier ----
        float* i0 = smem;                                     // image(s)
        float* i1 = smem + S2T2_IMG;                          // receives image(s+1)
        decode(lt);
        {
            const char* ws = w_base(lt, 0);
            const char* ib = uniform_ptr(in_base(lt, 0));
            static_for<0, 3>([&](auto dc) __attribute__((always_inline)) {
                static_for<0, 3>([&](auto yc) __attribute__((always_inline)) { load_wr(dc, yc, ws); });
            });
            static_for<0, S2T2_NDMA>([&](auto kc) __attribute__((always_inline)) { issue_in_dma(kc, ib, i0); });
        }
        zero_acc();
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
        // (the compiler's own wait counts enter the loop with nothing pending: merged with the prologue's issue order, every step would open
        // on vmcnt(0) -- behind the fragment loads the previous step issued last)
#pragma unroll
        for (int i = 0; i < 18; ++i) asm volatile("" : "+v"(wr[i / 6][(i / 2) % 3][i % 2]));
        while (true) {
            const bool last_ch = cs.ch + 1 == nchunk;
            const Cur cn = adv(cs);                           // the next step: its image and weight fragments are requested during this one
            auto prep = [&]() __attribute__((always_inline)) {
                if (last_ch && cn.tile < total) {
                    lt = origin(cn.tile);
                    decode(lt);
                }
                // (past the last tile: the last tile's first chunk again -- valid addresses, never used)
                ib_s = uniform_ptr(in_base(lt, cn.ch));
                wsrc_s = w_base(lt, cn.ch);
            };
            mfma_step2(i0, i1, prep);
            // this wave's share of image(s+1) has landed (the count: mfma_step2); the epilogue's stores come behind the wait, not into its count
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(S2T2_AFTER) : "memory");
            if (last_ch) {
                epilogue(cur);
                zero_acc();
                cur = lt;
                park(cur);
            }
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");      // every wave is done reading image(s) and has filled its share of image(s+1)
            if (cn.tile >= total) break;
            cs = cn;
            float* t = i0;
            i0 = i1;
            i1 = t;
        }
    } else {
        // ---- one image: two barriers per step ----
        float* w0 = smem + S2T_W_OFF;                             // weights(s)
        float* w1 = w0 + S2T_W;                                   // receives weights(s+1)
        // prologue: weights(0) by DMA, image(0) through the register set
        decode(lt);
        {
            const char* ws = w_base(lt, 0);
            const char* ib = in_base(lt, 0);
            static_for<0, S2T_NWT>([&](auto kc) __attribute__((always_inline)) { issue_dma(kc, ws, w0); });
            static_for<0, S2T_NIN>([&](auto kc) __attribute__((always_inline)) { issue_load(kc, ib); });
        }
        zero_acc();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        write_in();
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
        while (true) {
            const bool last_ch = cs.ch + 1 == nchunk;
            const Cur cn = adv(cs);                               // the next step: its units and weights are requested during this one
            auto prep = [&]() __attribute__((always_inline)) {
                if (last_ch && cn.tile < total) {
                    lt = origin(cn.tile);
                    decode(lt);
                }
                // (past the last tile: the last tile's first chunk again -- valid addresses, never used)
                ib_s = in_base(lt, cn.ch);
                wsrc_s = w_base(lt, cn.ch);
            };
            mfma_step(w0, w1, prep);
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");          // every wave is done reading image(s)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                          // this thread's units and weight DMA of s+1 have landed
            write_in();
            if (last_ch) {
                epilogue(cur);
                zero_acc();
                cur = lt;
                park(cur);
            }
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");          // image(s+1) is written, weights(s+1) are in LDS
            if (cn.tile >= total) break;
            cs = cn;
            float* t = w0;
            w0 = w1;
            w1 = t;
        }
    }
    if constexpr (D2) {
        // (word_v: the descriptor's range-guard word; this raising site is in the table of tests/test_hip_range_guard.py and probed element by
        // element, and across the tile walk, by its test_s2_tall_guard_* tests)
        if (word_v && !amax.at_most(65504.0f)) atomicOr(word_v, YOND_STATUS_HALF_OVERFLOW);   // an h half became +-inf
    }
    if (clk_on) {
        atomicAdd(clk_v, __builtin_amdgcn_s_memtime() - clk_c0);
        atomicAdd(clk_v + 1, __builtin_amdgcn_s_memrealtime() - clk_r0);
    }
}

template <bool D2>
__global__ __launch_bounds__(512) void conv_s2_tall_kernel(const YondConvDesc d) {
    s2t_body<D2, true>(d);
}
template <bool D2>
__global__ __launch_bounds__(512) void conv_s2_tall_kernel_one_image(const YondConvDesc d) {
    s2t_body<D2, false>(d);
}

// 1: a descriptor this file takes
static bool s2t_takes(const YondConvDesc& d) {
    if (d.ksize != 3 || d.stride != 2 || d.shuffle != 0 || d.tn != 64 || !d.src0 || d.src1 || d.C1 != 0 || !d.dst || !d.wpk) return false;
    if (d.in_fmt != YOND_FMT_SPLIT_PLANES || d.out_fmt != YOND_FMT_PLANES4 || d.res_fmt || d.res || d.out4_dst || d.pre_act) return false;
    if (d.post_act != 0 && d.post_act != 2) return false;
    if (d.N <= 0 || d.H <= 0 || d.W <= 0 || d.Ho != (d.H + 1) / 2 || d.Wo != (d.W + 1) / 2) return false;
    if (d.C0 <= 0 || d.C0 % 16 || d.Cout <= 0 || d.Cout % 64) return false;
    if ((long long)(d.ebatch ? d.N : 1) * d.Cout > S2T_FILM) return false;        // (the vectors of every image stay in LDS)
    if ((long long)d.N * d.H * d.W > 0x7fffffffLL) return false;
    // 32-bit offsets: elements over the whole input (as the template's dispatcher asks of register-staged split planes), bytes inside a chunk's planes
    if ((long long)d.N * (d.C0 / 16) * 4 * YOND_SP_PLANE_UNITS(d.H, d.W) * 4 >= 0x7fffffffLL) return false;
    if ((long long)YOND_SP_PLANE_UNITS(d.H, d.W) * 16 * 4 >= 0x7fffffffLL) return false;
    const long long tiles = (long long)(d.Cout / 64) * ((d.Wo + 31) / 32) * ((d.Ho + S2T_TH - 1) / S2T_TH) * d.N;
    if (tiles > 0x7fffffffLL) return false;
    if (d.Wo <= 16) {
        // what the template serves with folded tiles (conv_split.hip, stride 2) stays there
        const int f = d.Wo <= 8 ? 4 : 2;
        const long long subs = (long long)d.N * ((d.Ho + 3) / 4) * ((d.Wo + 32 / f - 1) / (32 / f));
        const long long tiles_f = (long long)(d.Cout / 64) * ((subs + f - 1) / f), tiles4 = (long long)(d.Cout / 64) * ((d.Ho + 3) / 4) * d.N;
        const bool fits = (long long)d.H * d.W * d.C0 * 4 * f < (1LL << 31);
        if (fits && (tiles_f + 255) / 256 < (tiles4 + 255) / 256) return false;
    }
    return true;
}

extern "C" int yond_conv_s2_tall_supported(const YondConvDesc* d) { return (d && (d->algo == 3 || d->algo == 7) && s2t_takes(*d)) ? 1 : 0; }

template <bool D2, bool TWO>
static int launch_s2t(const YondConvDesc& d, hipStream_t st) {
    static bool attr_set = false;
    constexpr int SMEM = TWO ? S2T2_SMEM : S2T_SMEM;
    auto kern = TWO ? conv_s2_tall_kernel<D2> : conv_s2_tall_kernel_one_image<D2>;
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, SMEM);
        if (e != hipSuccess) return (int)e;
        attr_set = true;
    }
    const long long total = (long long)(d.Cout / 64) * ((d.Wo + 31) / 32) * ((d.Ho + S2T_TH - 1) / S2T_TH) * d.N;
    const int grid = total < 256 ? (int)total : 256;         // one persistent workgroup per CU
    hipLaunchKernelGGL(kern, dim3(grid), dim3(512), SMEM, st, d);
    YOND_LAUNCH_CHECK();
    return YOND_OK;
}

// called by yond_conv2d_f32 (conv.hip) for desc.algo == 7; a descriptor it does not take is an error, not a fall-back (the caller asks
// yond_conv_s2_tall_supported first and keeps algo 3 otherwise)
int yond_conv_s2_tall_dispatch(const YondConvDesc& d, hipStream_t st) {
    if (!s2t_takes(d)) return YOND_EUNSUPPORTED;
    // Two chunks per tile (32 input channels: the layer 0 -> 1, whose time is mostly its 0.58 GB) stay on the one-image form: the two-image form's
    // 9 - 11 us there are inside the one-image form's own spread; every other depth takes two images (profiles/s2_two_image_ab.txt, section 2)
    bool two = d.C0 != 32;
#ifdef YOND_EXPERIMENTS         // both forms in one process, whatever the depth: YOND_S2T_FORM = 1 one image, 2 two images, 0 the shipped choice
    const long form = yond_exp_long("YOND_S2T_FORM", 0);
    if (form == 1 || form == 2) two = form == 2;
#endif
    if (two) return d.dst2 ? launch_s2t<true, true>(d, st) : launch_s2t<false, true>(d, st);
    return d.dst2 ? launch_s2t<true, false>(d, st) : launch_s2t<false, false>(d, st);
}
