// K1w: the decoder's 1x1 pixel-shuffle GEMM with STATIONARY weights, fed straight from split planes (descriptor algo 6).
//
// The same arithmetic as the K1 form of conv_split_kernel.h (its header: split operands, three v_mfma_f32_32x32x16_f16 per chunk, two
// accumulators) and, per accumulator, the same MFMA sequence -- bit-identical results -- with another data flow:
//   * a 1x1 GEMM has no halo and no tap reuse, and a split-plane unit (8 halves of one pixel and one channel half) already IS a lane's
//     B operand (conv_split_kernel.h, operand map): pixels go global -> VGPR by global_load_dwordx4, never through LDS;
//   * a persistent 512-thread workgroup serves ONE 64-wide channel tile for its whole life: the tile's weights (all K chunks, in the order
//     yond_pack_conv_split_weight_f32 writes them -- [chunk][channel half][part][64][8 halves]) are copied into LDS once, behind one
//     barrier; the A fragments are read from there with ds_read_b128 in the template's conflict-free layout;
//   * no barrier after that: a wave owns whole 32-pixel segments (32 pixels x 64 channels, two 32-channel blocks) and keeps a ring of D chunks
//     (2 D units per lane) in flight, refilled across segment boundaries; the waves drift apart and cover each other's latencies.
// The nct workgroups that read the same pixels (the sibling channel tiles) carry the same blockIdx % 8 -- one XCD, one L2 -- and walk the
// same segments in the same order.
// Covered: shuffle 1 with split-plane inputs (the low-resolution tensor, 2 Cr channels, and the skip tensor at the output resolution, Cr
// channels) and planes-of-4 output, Cr = 64 or 128 -- the decoder levels 2 -> 1 and 3 -> 2 --, and shuffle 2 (two sub-positions per tile) at
// Cr = 32 with the [N][H][W][C] store -- level 1 -> 0.  Everything else stays on the template (yond_gemm_k1_stationary_supported).  A consumer of finished planes, it raises no range flag (conv_split_kernel.h, range guard).
#include "common.h"

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// NCH: 16-channel chunks of K; NLO: those of the low-resolution input (the rest: the skip tensor); D: chunks in flight per wave
// S2: the two-sub-positions form (descriptor shuffle 2, conv_split_kernel.h S2) at 32-channel output pixels: the tile's two 32-column blocks are the sub-positions
// (dy, 0) and (dy, 1), the skip tensor's K range is [its chunks at dx = 0 | the same at dx = 1 | zero-weight chunks, read at dx = 0, chunk 0]; [N][H][W][C] store
template <int NCH, int NLO, int D, bool S2 = false>
__global__ __launch_bounds__(512) void gemm_k1_stationary_kernel(const YondConvDesc d) {
    constexpr int WS = NCH % 2 == 0 ? 2 : 3;                     // sets of A fragments (one chunk ahead; the rotation closes at the segment's end)
    static_assert(NCH % D == 0 && NCH % WS == 0 && D >= 2 && NLO > 0 && NLO < NCH, "the ring holds whole rounds of a segment's chunks");
    constexpr int NHI = NCH - NLO;
    constexpr int CRC = S2 ? NHI / 2 : NHI;                      // chunks of the skip tensor
    constexpr int FILM_OFF = NCH * 1024, EP_OFF = FILM_OFF + 16 * 128, EPS = 36;     // floats: scale / shift vectors; S2: per wave a 32-pixel x 36-float transpose scratch
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, lh = lane >> 5;
    const int Cr = d.Cout / 4, nct = d.Cout / 64;
    // blocks with the same blockIdx % 8 share an XCD: its per_xcd blocks are per_xcd / nct groups of nct sibling tiles
    const int per_xcd = gridDim.x / 8;
    const int bx = blockIdx.x % 8, bj = blockIdx.x / 8;
    const int ct = bj % nct, grp = bx * (per_xcd / nct) + bj / nct, ngrp = gridDim.x / nct;
    const bool clk_on = d.clk != nullptr && blockIdx.x == 0 && tid == 0;       // measurement aid (YondConvDesc.clk)
    unsigned long long clk_c0 = 0, clk_r0 = 0;
    if (clk_on) { clk_c0 = __builtin_amdgcn_s_memtime(); clk_r0 = __builtin_amdgcn_s_memrealtime(); }

    // the tile's weights and its scale / shift vectors (one pair per image with ebatch), once
    {
        const f32x4* wsrc = (const f32x4*)(d.wpk + (size_t)ct * NCH * 1024);
        f32x4* wl = (f32x4*)smem;
        for (int i = tid; i < NCH * 256; i += 512) wl[i] = wsrc[i];
        float* film = smem + FILM_OFF;
        const int nfilm = d.ebatch ? d.N : 1;
        for (int i = tid; i < nfilm * 128; i += 512) {
            const int im = i >> 7, k = i & 127;
            const int cb = (ct * 64 + (k & 63)) % Cr;
            film[i] = k < 64 ? (d.escale ? d.escale[im * Cr + cb] : 1.0f) : (d.eshift ? d.eshift[im * Cr + cb] : 0.0f);
        }
    }
    __syncthreads();

    const int nsx = (d.W + 31) / 32;
    const long long nseg = (long long)d.N * d.H * nsx;
    const long long sstep = 8LL * ngrp;
    const long long s0 = grp + (long long)ngrp * wave;
    if (s0 < nseg) {
        const bool rev = d.tile_order != 0;                      // (the same segments, last first: results do not depend on it)
        const size_t PS0 = (size_t)YOND_SP_PLANE_UNITS(d.H, d.W) * 16, PS1 = (size_t)YOND_SP_PLANE_UNITS(2 * d.H, 2 * d.W) * 16;   // bytes per plane
        // the tile's sub-position (dy, dx) and first channel of the output pixel (S2, 32-channel pixels: tile = dy, its blocks = dx 0 and 1)
        const int sp = S2 ? 2 * ct : (ct * 64) / Cr, cb0 = S2 ? 0 : (ct * 64) % Cr;
        const int Hout = 2 * d.H, Wout = 2 * d.W;
        const float slope_eff = d.post_act == 2 ? d.slope : 1.0f;
        struct Geo { int n, y, x; unsigned vlo, vhi, vhi1; };
        auto geo = [&](long long s) {
            Geo g;
            const long long t = rev ? nseg - 1 - s : s;
            const int per = d.H * nsx;
            g.n = (int)(t / per);
            const int r = (int)(t - (long long)g.n * per);
            g.y = r / nsx;
            g.x = (r - g.y * nsx) * 32 + li;
            const bool in = g.x < d.W;
            // byte offset of the lane's unit from the plane (chunk, half 0, part h): the zero unit behind the plane for a pixel outside the image
            g.vlo = (unsigned)((size_t)lh * 2 * PS0) + (unsigned)(in ? g.y * d.W + g.x : d.H * d.W) * 16u;
            g.vhi = (unsigned)((size_t)lh * 2 * PS1) + (unsigned)(in ? (2 * g.y + (sp >> 1)) * Wout + 2 * g.x + (sp & 1) : Hout * Wout) * 16u;
            g.vhi1 = in ? g.vhi + 16u : g.vhi;                   // S2: the neighbouring output pixel (dx = 1) is the next unit; the zero unit stays where it is
            return g;
        };
        f16x8 ring[D][2];
        auto issue = [&](auto cc, const Geo& g) __attribute__((always_inline)) {
            constexpr int c = decltype(cc)::value, slot = c % D;
            if constexpr (c < NLO) {
                const char* b = (const char*)d.src0 + ((size_t)g.n * NLO + c) * 4 * PS0;
                ring[slot][0] = *(const f16x8*)(b + g.vlo);
                ring[slot][1] = *(const f16x8*)(b + PS0 + g.vlo);
            } else {
                constexpr int k = c - NLO, q = S2 ? k / CRC : 0;
                constexpr int ch = q < 2 ? k - q * CRC : 0;        // (S2: [dx = 0 | dx = 1 | zero-weight chunks: dx = 0, chunk 0])
                const char* b = (const char*)d.src1 + ((size_t)g.n * CRC + ch) * 4 * PS1;
                const unsigned v = q == 1 ? g.vhi1 : g.vhi;
                ring[slot][0] = *(const f16x8*)(b + v);
                ring[slot][1] = *(const f16x8*)(b + PS1 + v);
            }
        };
        typedef const __attribute__((address_space(3))) f16x8* lds_h8;
        const __attribute__((address_space(3))) float* wb = (const __attribute__((address_space(3))) float*)(smem + (lh * 2 * 64 + li) * 4);
        const float* film = smem + FILM_OFF;
        // (the dispatcher keeps dst below 2^31 bytes: byte offsets in 32 bits, bit 31 = beyond the extent)
        const unsigned hw_out = (unsigned)(Hout * Wout);
        const __amdgpu_buffer_rsrc_t orsrc = __builtin_amdgcn_make_buffer_rsrc(d.dst, 0, (int)((unsigned)d.N * (unsigned)Cr * hw_out * 4u), 0x00020000);
        f16x8 wt[WS][2][2];                                      // A fragments of a chunk [c % WS][32-channel block][part], read one chunk ahead
        auto load_w = [&](auto cc) __attribute__((always_inline)) {
            constexpr int c = decltype(cc)::value;
#pragma unroll
            for (int nn = 0; nn < 2; ++nn)
#pragma unroll
                for (int p = 0; p < 2; ++p) wt[c % WS][nn][p] = *(lds_h8)(wb + ((c * 4 + p) * 64 + nn * 32) * 4);
        };

        // one segment: its NCH chunks (chunk c + D -- of this segment or of the next -- requested behind chunk c's MFMAs), then the store
        auto segment = [&](const Geo& cur, const Geo& nxt) __attribute__((always_inline)) {
            f32x16 acc[2][2];                                    // [0] h_w h_x ; [1] the two cross terms (carry the 2^11 scale)  x  32-channel block
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int nn = 0; nn < 2; ++nn)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[a][nn][r] = 0.0f;
            static_for<0, NCH>([&](auto cc) __attribute__((always_inline)) {
                constexpr int c = decltype(cc)::value, slot = c % D, ws = c % WS;
                load_w(IntC<(c + 1) % NCH>{});                   // the next chunk's A fragments (past the segment's end: chunk 0 again, for the next segment)
                const f16x8 xh = ring[slot][0], xl = ring[slot][1];
                // the template's order: h_w l_x, then h_w h_x, then l_w h_x
#pragma unroll
                for (int nn = 0; nn < 2; ++nn) acc[1][nn] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wt[ws][nn][0], xl, acc[1][nn], 0, 0, 0);
#pragma unroll
                for (int nn = 0; nn < 2; ++nn) acc[0][nn] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wt[ws][nn][0], xh, acc[0][nn], 0, 0, 0);
#pragma unroll
                for (int nn = 0; nn < 2; ++nn) acc[1][nn] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wt[ws][nn][1], xh, acc[1][nn], 0, 0, 0);
                if constexpr (c + D < NCH) issue(IntC<c + D>{}, cur);
                else issue(IntC<c + D - NCH>{}, nxt);
                // (left to itself the scheduler hoists a whole segment's loads to its top and spills hundreds of registers: a chunk's instructions stay in the chunk)
                __builtin_amdgcn_sched_barrier(0);
            });
            // store, lane = pixel, into planes of 4 channels: the operations of the template's epilogue_direct in its order.  Through a buffer
            // resource over dst: a lane outside the image stores beyond its extent, which the hardware drops -- no branch around the stores, so the
            // compiler's count of the operations in flight stays exact across the segment boundary (behind a branch it drained the ring to two chunks)
            if constexpr (S2) {
                // [N][H][W][C] store: each 32-pixel x 32-channel block goes through the wave's private LDS scratch and is read back with 8 lanes per
                // pixel (a store instruction then covers whole 128-byte pixels) -- the template's transposed epilogue, its operations in its order
                float* sw = smem + EP_OFF + wave * (32 * EPS);
                const int pj = lane >> 3, u = lane & 7;              // read-back: pixel pj + 8 j, channels 4 u .. 4 u + 3
                const int x0 = cur.x - li;
                const unsigned rowb = (unsigned)((cur.n * Hout + 2 * cur.y + (sp >> 1)) * Wout + 2 * x0);
                const float* fv = film + (d.ebatch ? cur.n * 128 : 0) + 4 * u;
#pragma unroll
                for (int nn = 0; nn < 2; ++nn) {
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        f32x4 v;
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = fmaf(acc[1][nn][4 * g + e], 1.0f / 2048.0f, acc[0][nn][4 * g + e]);
                        *(f32x4*)(sw + li * EPS + 8 * g + 4 * lh) = v;
                    }
                    const f32x4 es = *(const f32x4*)(fv + nn * 32), et = *(const f32x4*)(fv + 64 + nn * 32);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int pp = pj + 8 * j;
                        const f32x4 x = *(const f32x4*)(sw + pp * EPS + 4 * u);
                        f32x4 v;
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            float y = fmaf(x[e], es[e], et[e]);
                            y = y > 0.0f ? y : y * slope_eff;
                            v[e] = y + 0.0f;
                        }
                        const unsigned off = (((rowb + 2u * (unsigned)pp + (unsigned)nn) * 32u + 4u * (unsigned)u) * 4u) | (x0 + pp < d.W ? 0u : 0x80000000u);
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), orsrc, (int)off, 0, 0);
                    }
                }
                return;
            }
            const unsigned pixo = (unsigned)((2 * cur.y + (sp >> 1)) * Wout + 2 * cur.x + (sp & 1));
            const unsigned mask = cur.x < d.W ? 0u : 0x80000000u;
            const float* fv = film + (d.ebatch ? cur.n * 128 : 0) + 4 * lh;
#pragma unroll
            for (int nn = 0; nn < 2; ++nn) {
                const int cbase = cb0 + nn * 32 + 4 * lh;
                const unsigned ob = (((unsigned)(cur.n * (Cr / 4) + cbase / 4) * hw_out + pixo) * 16u) | mask;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 es = *(const f32x4*)(fv + nn * 32 + 8 * g), et = *(const f32x4*)(fv + 64 + nn * 32 + 8 * g);
                    f32x4 v;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float x = acc[0][nn][4 * g + e];
                        x = fmaf(acc[1][nn][4 * g + e], 1.0f / 2048.0f, x);
                        x = fmaf(x, es[e], et[e]);
                        x = x > 0.0f ? x : x * slope_eff;
                        v[e] = x + 0.0f;
                    }
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), orsrc, (int)(ob + (unsigned)g * 32u * hw_out), 0, 0);
                }
            }
        };

        Geo cur = geo(s0);
        static_for<0, D>([&](auto cc) { issue(cc, cur); });
        load_w(IntC<0>{});
        long long sn = s0 + sstep;
        // (the first segment apart from the loop: the loop's head is then entered with the same operations in flight from both sides -- D chunks and the
        // previous segment's stores -- and the compiler's counted waits stay exact)
        Geo nxt = sn < nseg ? geo(sn) : cur;
        segment(cur, nxt);
        while (sn < nseg) {
            cur = nxt;
            sn += sstep;
            nxt = sn < nseg ? geo(sn) : cur;                     // (past the end: the last segment's units again, never used)
            segment(cur, nxt);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // the look-ahead loads past the end
    }
    if (clk_on) {
        atomicAdd(d.clk, __builtin_amdgcn_s_memtime() - clk_c0);
        atomicAdd(d.clk + 1, __builtin_amdgcn_s_memrealtime() - clk_r0);
    }
}

// NCH of a descriptor this file takes (24 / 12: shuffle 1, planes of 4 out; 9: shuffle 2 at 32-channel output pixels, [N][H][W][C] out), or 0
static int k1s_chunks(const YondConvDesc& d) {
    if (d.ksize != 1 || d.stride != 1 || (d.shuffle != 1 && d.shuffle != 2) || d.tn != 64 || !d.src0 || !d.src1 || !d.dst || !d.wpk) return 0;
    if (d.in_fmt != YOND_FMT_SPLIT_PLANES || d.res_fmt || d.res || d.dst2 || d.out4_dst || d.pre_act) return 0;
    if (d.out_fmt != (d.shuffle == 2 ? YOND_FMT_NHWC_F32 : YOND_FMT_PLANES4)) return 0;
    if (d.post_act != 0 && d.post_act != 2) return 0;
    if (d.Ho != d.H || d.Wo != d.W || d.N <= 0 || d.H <= 0 || d.W <= 0 || d.Cout <= 0 || d.Cout % 128) return 0;
    const int Cr = d.Cout / 4, nct = d.Cout / 64;
    if (d.shuffle == 2) {
        if (Cr != 32 || d.C0 != 64 || d.C1 != 80) return 0;          // [64 low-resolution | 32 at dx = 0 | 32 at dx = 1 | one zero chunk]
    } else if (d.Cout % 256 || 32 % nct || d.C0 != 2 * Cr || d.C1 != Cr) return 0;         // (sibling tiles fill whole XCD shares of the 256 workgroups)
    if (d.ebatch && d.N > 16) return 0;                             // (the vectors of every image stay in LDS)
    if ((long long)d.N * d.H * d.W > 0x7fffffffLL) return 0;
    if ((long long)d.N * Cr * 4 * d.H * d.W * 4 >= 0x7fffffffLL) return 0;          // dst: 32-bit byte offsets through a buffer resource
    // 32-bit unit offsets inside a chunk's four planes (as the template's dispatcher asks of its split-plane inputs)
    if ((long long)YOND_SP_PLANE_UNITS(d.H, d.W) * 4 * 16 * 4 >= 0x7fffffffLL) return 0;
    const int nch = (d.C0 + d.C1) / 16;
    if (d.shuffle == 2) return nch == 9 ? nch : 0;
    return (nch == 24 || nch == 12) ? nch : 0;
}

extern "C" int yond_gemm_k1_stationary_supported(const YondConvDesc* d) { return (d && (d->algo == 3 || d->algo == 6) && k1s_chunks(*d)) ? 1 : 0; }

template <int NCH, int NLO, int D, bool S2 = false>
static int launch_k1s(const YondConvDesc& d, hipStream_t st) {
    constexpr int SMEM = (NCH * 1024 + 16 * 128 + (S2 ? 8 * 32 * 36 : 0)) * 4;
    static_assert(SMEM <= 160 * 1024, "LDS budget");
    static bool attr_set = false;
    auto kern = gemm_k1_stationary_kernel<NCH, NLO, D, S2>;
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, SMEM);
        if (e != hipSuccess) return (int)e;
        attr_set = true;
    }
    // gfx950 (MI355X): 256 CUs in 8 XCDs, workgroups dealt to the XCDs round-robin -- one persistent workgroup per CU, blockIdx % 8 = the XCD share
    // (the kernel's sibling-tile grouping; k1s_chunks admits only tile counts that divide an XCD's 32 workgroups).  Placement changes speed only.
    constexpr int K1S_GRID = 256;
    static_assert(K1S_GRID % 8 == 0, "whole XCD shares");
    hipLaunchKernelGGL(kern, dim3(K1S_GRID), dim3(512), SMEM, st, d);
    YOND_LAUNCH_CHECK();
    return YOND_OK;
}

// called by yond_conv2d_f32 (conv.hip) for desc.algo == 6; a descriptor it does not take is an error, not a fall-back (the caller asks
// yond_gemm_k1_stationary_supported first and keeps algo 3 otherwise)
int yond_gemm_k1_stationary_dispatch(const YondConvDesc& d, hipStream_t st) {
    const int nch = k1s_chunks(d);
#ifdef YOND_EXPERIMENTS         // ring depths beside the shipped ones (profiles/k1_stationary_ab.txt, section 5)
    const long depth = yond_exp_long("YOND_K1S_DEPTH", 0);
    if (nch == 24 && depth == 4) return launch_k1s<24, 16, 4>(d, st);
    if (nch == 24 && depth == 8) return launch_k1s<24, 16, 8>(d, st);       // (depth 12 at 24 chunks spills: 28 bytes of scratch)
    if (nch == 12 && depth == 4) return launch_k1s<12, 8, 4>(d, st);
    if (nch == 12 && depth == 12) return launch_k1s<12, 8, 12>(d, st);
    if (nch == 9 && depth == 3) return launch_k1s<9, 4, 3, true>(d, st);
#endif
    if (nch == 24) return launch_k1s<24, 16, 6>(d, st);
    if (nch == 12) return launch_k1s<12, 8, 6>(d, st);
    if (nch == 9) return launch_k1s<9, 4, 9, true>(d, st);
    return YOND_EUNSUPPORTED;
}
