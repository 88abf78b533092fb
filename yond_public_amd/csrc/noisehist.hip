// M3: residual histograms for the noise-model KL divergence (utils/sidd_utils.py:280-304 get_histogram / cal_kld).  The contract is in
// include/yond_hip.h.  House rules: asynchronous on the caller's stream, no allocation or synchronisation in the launch functions, no
// scratch, no device printf / assert.
//   noise_hist      r = noisy - clean (one float32 subtraction), binned by np.histogram's rule on the UPLOADED float64 edges, split by the
//                   clean value's intensity band and the pixel's CFA position: 8 B read per pixel.
//   pg_noise_hist   the same binning of r = pg_element(clean) - clean, the value yond_pg_noise_f32 would have stored (pgnoise_element.h:
//                   one definition for both kernels), without storing it: 4 B read per pixel, bound by the sampler's arithmetic.
// The bin: a guess from the caller's hint, floor((r - hint_lo) * hint_inv) + 1 in float32 clamped to the bins, then SETTLED against the edges in LDS
// (walk down while r < edges[g], up while r >= edges[g + 1]): the hint decides how many comparisons are made, never the bin.  The
// reference's inner edges come from np.arange and are not -R + i * bw to the last bit (the middle one is 8.3e-17): a float32 residual on
// such an edge is what the settling is for.
// Privatisation: residuals of a natural frame fall into two or three central bins, so a workgroup's LDS histogram is kept in R = 2^k
// replicas, bin-major (s_h[bin * R + (lane & (R - 1))]): R = 32 for the default 4 x 66 bins puts the 32 lanes of a half-wave on 32 banks
// whatever bins they hit, and two lanes at most on one address.  R halves as the bands multiply the bins (NH_SLOTS counters in all).
// The fused kernel keeps R <= 4: the sampler's arithmetic sets its pace (an LDS atomic that waits a few dozen cycles is lost in it), and
// 4 KiB of LDS instead of 33 leave the registers to decide the occupancy.  The LDS is dynamic: edges, histogram, thresholds.
// One flush per workgroup: lane t adds the replicas of the bins t, t + 256, ... (rotated by its lane number: conflict-free) and makes one
// 64-bit device-scope atomic add per NON-ZERO bin -- a hundred or so per workgroup, from a persistent grid capped at
// YOND_NOISEHIST_MAX_BLOCKS (the fused kernel: YOND_NOISEHIST_MODEL_MAX_BLOCKS) with a stride loop.  Counts are integers: the result does
// not depend on the schedule.
#include "common.h"
#include "pgnoise_element.h"

#define NH_T 256
#define NH_SLOTS 8448                       /* most counters a workgroup keeps: 32 replicas of 4 x 66 bins, 33 KiB */
// measured alternatives: tools/noisekld_bench.py, DESIGN section 4 "M3"
#define NH_RSHIFT_HIST 5                    /* log2 of the most replicas of the histogram kernel */
#define NH_RSHIFT_MODEL 2                   /* ... of the fused kernel: the sampler sets its pace, a small histogram leaves it the occupancy */
#define NH_UNROLL 2                         /* vectors per array a lane of the histogram kernel has in flight */

static_assert(YOND_NOISEHIST_BLOCK_ELEMS == 4 * NH_T, "a workgroup's pass: one vector of 4 per lane");

struct NHParams {
    const double* edges;        // [nbin + 1], ascending
    const float* thr;           // [nb - 1], ascending; null when nb == 1
    int nbin, nb;
    double hint_lo, hint_inv;
    int rshift;                 // log2(replicas)
    unsigned long long* counts; // [B][nb][4][nbin]
};

// the workgroup's LDS (dynamic): the edges, the replicated histogram, the thresholds
struct NHShared {
    const double* e;            // [nbin + 1]
    unsigned* h;                // [4 nb nbin << rshift]
    const float* t;             // [nb - 1]
    double e_first, e_last;     // edges[0], edges[nbin]: in registers
    float hint_lo, hint_inv;
};

// one pixel: residual r, clean value cl, CFA position c.  Uncounted: r NaN, +-inf or outside [edges[0], edges[nbin]].
__device__ __forceinline__ void nh_count(const NHShared& s, const NHParams& p, unsigned rep, float r, float cl, unsigned c) {
    unsigned b = 0;
    for (int k = 0; k < p.nb - 1; ++k) b += s.t[k] <= cl ? 1u : 0u;          // a NaN clean value: band 0
    if (!(fabsf(r) <= 3.402823466e38f)) return;                              // NaN, +-inf
    const double rd = (double)r;
    const int last = p.nbin - 1;
    if (!(rd >= s.e_first && rd <= s.e_last)) return;
    const float t = floorf((r - s.hint_lo) * s.hint_inv) + 1.0f;              // the guess, in float32: it decides nothing
    int g = (int)fminf(fmaxf(t, 0.0f), (float)last);                          // (fmaxf drops a NaN guess: bin 0)
    while (g > 0 && rd < s.e[g]) --g;
    while (g < last && rd >= s.e[g + 1]) ++g;                                 // the last bin keeps r == edges[nbin]
    atomicAdd(&s.h[((((b << 2) + c) * (unsigned)p.nbin + (unsigned)g) << p.rshift) + rep], 1u);
}

// MODEL 0: r = noisy - clean.  MODEL 1: r = pg_element(clean) - clean, `noisy` unused.  VEC: 16-byte loads (W % 4 == 0, pointers aligned).
template <int MODEL, int VEC>
__global__ __launch_bounds__(NH_T, 6) void noise_hist_kernel(const float* __restrict__ noisy, const float* __restrict__ clean, unsigned n,
                                                          unsigned W, const YondPGItem* __restrict__ items, int clip, NHParams p) {
    extern __shared__ double nh_lds[];
    const unsigned tid = threadIdx.x;
    const unsigned fb = blockIdx.y;
    const unsigned total = 4u * (unsigned)p.nb * (unsigned)p.nbin;
    double* s_e = nh_lds;
    unsigned* s_h = reinterpret_cast<unsigned*>(s_e + p.nbin + 1);
    float* s_t = reinterpret_cast<float*>(s_h + (total << p.rshift));
    for (unsigned i = tid; i <= (unsigned)p.nbin; i += NH_T) s_e[i] = p.edges[i];
    if ((int)tid < p.nb - 1) s_t[tid] = p.thr[tid];
    for (unsigned i = tid; i < (total << p.rshift); i += NH_T) s_h[i] = 0u;
    const NHShared s = {s_e, s_h, s_t, p.edges[0], p.edges[p.nbin], (float)p.hint_lo, (float)p.hint_inv};
    __syncthreads();

    const unsigned rep = tid & ((1u << p.rshift) - 1u);
    const float* cl = clean + (size_t)fb * n;
    const float* ny = MODEL ? nullptr : noisy + (size_t)fb * n;
    YondPGItem it = {};
    if (MODEL) it = items[fb];
    const unsigned stride = gridDim.x * NH_T;
    if (VEC) {
        const unsigned nvec = n >> 2;                                        // W % 4 == 0: a vector lies in one row, from an even column
        if (MODEL) {
            for (unsigned v = blockIdx.x * NH_T + tid; v < nvec; v += stride) {
                const unsigned i0 = v << 2;
                f32x4 x = *reinterpret_cast<const f32x4*>(cl + i0), r = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 1
                for (unsigned u = 0; u < 4; ++u) {                           // one copy of the sampler: x and r rotate through lanes 0 / 3
                    const float rv = pg_element(it, (uint64_t)(i0 + u), x[0], clip) - x[0];
                    x = f32x4{x[1], x[2], x[3], x[0]};
                    r = f32x4{r[1], r[2], r[3], rv};
                }
                const unsigned c0 = ((i0 / W) & 1u) << 1;                    // (four rotations: x is the vector again)
                nh_count(s, p, rep, r[0], x[0], c0);                         // the four together: their LDS reads overlap
                nh_count(s, p, rep, r[1], x[1], c0 + 1u);
                nh_count(s, p, rep, r[2], x[2], c0);
                nh_count(s, p, rep, r[3], x[3], c0 + 1u);
            }
        } else {
            for (unsigned v = blockIdx.x * NH_T + tid; v < nvec; v += stride * NH_UNROLL) {
                f32x4 X[NH_UNROLL], Y[NH_UNROLL];
#pragma unroll
                for (int u = 0; u < NH_UNROLL; ++u) {                        // every load issued before the first use
                    const unsigned vu = v + u * stride;                      // (v < 2^29, stride < 2^20: no wrap)
                    const unsigned idx = (vu < nvec ? vu : v) << 2;
                    X[u] = *reinterpret_cast<const f32x4*>(cl + idx);
                    Y[u] = *reinterpret_cast<const f32x4*>(ny + idx);
                }
#pragma unroll
                for (int u = 0; u < NH_UNROLL; ++u) {
                    const unsigned vu = v + u * stride;
                    if (vu < nvec) {
                        const unsigned c0 = (((vu << 2) / W) & 1u) << 1;
                        nh_count(s, p, rep, Y[u][0] - X[u][0], X[u][0], c0);
                        nh_count(s, p, rep, Y[u][1] - X[u][1], X[u][1], c0 + 1u);
                        nh_count(s, p, rep, Y[u][2] - X[u][2], X[u][2], c0);
                        nh_count(s, p, rep, Y[u][3] - X[u][3], X[u][3], c0 + 1u);
                    }
                }
            }
        }
    } else {
        for (unsigned i = blockIdx.x * NH_T + tid; i < n; i += stride) {
            const unsigned row = i / W, col = i - row * W;
            const float x = cl[i];
            const float yv = MODEL ? pg_element(it, (uint64_t)i, x, clip) : ny[i];
            nh_count(s, p, rep, yv - x, x, ((row & 1u) << 1) + (col & 1u));
        }
    }
    __syncthreads();

    const unsigned R = 1u << p.rshift;
    unsigned long long* out = p.counts + (size_t)fb * total;
    for (unsigned bin = tid; bin < total; bin += NH_T) {
        unsigned sum = 0;
        for (unsigned k = 0; k < R; ++k) sum += s_h[(bin << p.rshift) + ((k + tid) & (R - 1u))];
        if (sum) atomicAdd(out + bin, (unsigned long long)sum);
    }
}

// the checks both entry points share, and the launch
static int nh_launch(int model, const float* noisy, const float* clean, int B, int H, int W, const YondPGItem* items, int clip,
                     const double* edges, int ne, const float* thr, int nb, double hint_lo, double hint_inv, unsigned long long* counts,
                     void* stream) {
    if (!clean || !edges || !counts || (!model && !noisy) || (model && !items)) return YOND_EINVAL;
    if (B < 1 || B > 65535 || H < 2 || W < 2 || (H & 1) || (W & 1)) return YOND_EINVAL;
    if (ne < 2 || nb < 1 || (nb > 1 && !thr) || (clip != 0 && clip != 1)) return YOND_EINVAL;
    if ((((uintptr_t)clean) | ((uintptr_t)noisy) | ((uintptr_t)thr)) & 3u) return YOND_EINVAL;
    if ((((uintptr_t)edges) | ((uintptr_t)counts)) & 7u) return YOND_EINVAL;
    const size_t n = (size_t)H * (size_t)W;
    if (n > 0x7fffffffull) return YOND_EINVAL;                               // pixel indices (and their stride loop) and a workgroup's counters are 32-bit
    const int nbin = ne - 1;
    if (nbin > YOND_NOISEHIST_MAX_BINS || nb > YOND_NOISEHIST_MAX_BANDS) return YOND_EUNSUPPORTED;
    const size_t total = (size_t)4 * nb * nbin;
    if (total > NH_SLOTS) return YOND_EUNSUPPORTED;
    int rshift = 0;
    const int rmax = model ? NH_RSHIFT_MODEL : NH_RSHIFT_HIST;
    while (rshift < rmax && (total << (rshift + 1)) <= NH_SLOTS) ++rshift;
    const size_t lds = sizeof(double) * (size_t)ne + sizeof(unsigned) * (total << rshift) + sizeof(float) * (size_t)(nb - 1);
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(counts, 0, sizeof(unsigned long long) * total * (size_t)B, st);
    if (e != hipSuccess) return (int)e;
    const int vec = !((((uintptr_t)clean) | ((uintptr_t)noisy)) & 15u) && W % 4 == 0;
    size_t cap = (size_t)(model ? YOND_NOISEHIST_MODEL_MAX_BLOCKS : YOND_NOISEHIST_MAX_BLOCKS) / (size_t)B;
    if (cap < 1) cap = 1;
    size_t blocks = (n + YOND_NOISEHIST_BLOCK_ELEMS - 1) / YOND_NOISEHIST_BLOCK_ELEMS;
    if (blocks > cap) blocks = cap;
    NHParams p = {edges, thr, nbin, nb, hint_lo, hint_inv, rshift, counts};
    const dim3 grid((unsigned)blocks, (unsigned)B), block(NH_T);
#define NH_GO(M, V) hipLaunchKernelGGL((noise_hist_kernel<M, V>), grid, block, lds, st, noisy, clean, (unsigned)n, (unsigned)W, items, clip, p)
    if (model) {
        if (vec) NH_GO(1, 1); else NH_GO(1, 0);
    } else {
        if (vec) NH_GO(0, 1); else NH_GO(0, 0);
    }
#undef NH_GO
    YOND_LAUNCH_CHECK();
    return YOND_OK;
}

extern "C" int yond_noise_hist_f32(const float* noisy, const float* clean, int B, int H, int W, const double* edges, int ne,
                                   const float* thresholds, int nb, double hint_lo, double hint_inv, unsigned long long* counts,
                                   void* stream) {
    return nh_launch(0, noisy, clean, B, H, W, nullptr, 0, edges, ne, thresholds, nb, hint_lo, hint_inv, counts, stream);
}

extern "C" int yond_pg_noise_hist_f32(const float* clean, int B, int H, int W, const YondPGItem* items, int clip, const double* edges,
                                      int ne, const float* thresholds, int nb, double hint_lo, double hint_inv,
                                      unsigned long long* counts, void* stream) {
    return nh_launch(1, nullptr, clean, B, H, W, items, clip, edges, ne, thresholds, nb, hint_lo, hint_inv, counts, stream);
}
