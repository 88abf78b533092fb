// R2 / R3: the two ends of a full-frame run (data.py's host normalisation and its inverse), flat streaming kernels over n = H * W.
//   ingest  out[i] = ((float)raw[i] - bl) * ratio / scale        raw uint16 or float32 DN -> float32, optionally clamped to [0, 1]
//   emit    out[i] = (uint16) rint(min(max(x[i] * scale [/ ratio] + bl, 0), 65535))       float32 -> uint16 DN, + a saturation count
// House rules: asynchronous on the caller's stream, no allocation or synchronisation in the launch function, no scratch.
// Every float32 operation is rounded on its own (the build has -ffp-contract=off; the division is the IEEE one), in the order
// NumPy evaluates data.py's expression: the results are bit-equal to the host path (tests/rawio_model.py).
// One lane moves 16 bytes per access: RAWIO_V = 8 elements where one side is uint16 (one 16-byte access there, two on the float
// side), 4 for float32 -> float32.  The pointers need only element alignment (a frame sliced out of a stack starts 2 bytes off a
// 16-byte boundary): a scalar head of < V elements brings the STORES to a 16-byte boundary, the loads go through vector types of
// element alignment (unaligned global loads are legal on gfx950; where source and destination happen to agree they are aligned
// too), a scalar tail takes what is left.  grid = min(ceil(vectors / 256), 2048), grid-stride, 64-bit element indices.
#include "common.h"

#define RAWIO_T 256
#define RAWIO_MAX_BLOCKS 2048

typedef uint16_t u16x8 __attribute__((ext_vector_type(8)));
typedef uint16_t u16x8_u __attribute__((ext_vector_type(8), aligned(2)));      // element-aligned views for the loads
typedef float f32x4_u __attribute__((ext_vector_type(4), aligned(4)));

__device__ __forceinline__ float ingest_one(float v, float bl, float ratio, float scale, int clip01) {
    float x = v - bl;
    x = x * ratio;
    x = x / scale;
    if (clip01) x = x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x);       // np.clip: a NaN stays a NaN (fmaxf / fminf would return 0)
    return x;
}

// returns the DN; bad += 1 when the value was NaN or had to be clamped at either end
__device__ __forceinline__ uint16_t emit_one(float x, float bl, float scale, float ratio, int undo_gain, int& bad) {
    float y = x * scale;
    if (undo_gain) y = y / ratio;
    y = y + bl;
    const bool isnan_ = y != y, lo = y < 0.0f, hi = y > 65535.0f;
    bad += (isnan_ || lo || hi) ? 1 : 0;
    y = (isnan_ || lo) ? 0.0f : (hi ? 65535.0f : y);
    return (uint16_t)rintf(y);                                      // ties to even
}

__device__ __forceinline__ void load8(const uint16_t* p, float (&v)[8]) {
    const u16x8_u r = *reinterpret_cast<const u16x8_u*>(p);
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = (float)r[u];
}
__device__ __forceinline__ void load8(const float* p, float (&v)[8]) {
    const f32x4_u a = *reinterpret_cast<const f32x4_u*>(p), b = *reinterpret_cast<const f32x4_u*>(p + 4);
#pragma unroll
    for (int u = 0; u < 4; ++u) { v[u] = a[u]; v[4 + u] = b[u]; }
}

// V = 8 for uint16 in, 4 for float32 in; `head` scalar elements, then nvec vectors of V, then the scalar tail
template <typename T, int V>
__global__ __launch_bounds__(RAWIO_T) void raw_ingest_kernel(const T* __restrict__ raw, size_t n, size_t head, size_t nvec, float bl, float ratio,
                                                             float scale, int clip01, float* __restrict__ out) {
    if (blockIdx.x == 0 && threadIdx.x < 2 * V) {                   // head and tail: fewer than V elements each
        const size_t tail0 = head + nvec * V;
        const size_t i = threadIdx.x < V ? (size_t)threadIdx.x : tail0 + (threadIdx.x - V);
        const bool mine = threadIdx.x < V ? (size_t)threadIdx.x < head : i < n;
        if (mine) out[i] = ingest_one((float)raw[i], bl, ratio, scale, clip01);
    }
    const size_t step = (size_t)gridDim.x * RAWIO_T;
    for (size_t q = (size_t)blockIdx.x * RAWIO_T + threadIdx.x; q < nvec; q += step) {
        const size_t i = head + q * V;
        if constexpr (V == 8) {
            float v[8];
            load8(raw + i, v);
            f32x4 a, b;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                a[u] = ingest_one(v[u], bl, ratio, scale, clip01);
                b[u] = ingest_one(v[4 + u], bl, ratio, scale, clip01);
            }
            *reinterpret_cast<f32x4*>(out + i) = a;
            *reinterpret_cast<f32x4*>(out + i + 4) = b;
        } else {
            const f32x4_u r = *reinterpret_cast<const f32x4_u*>(raw + i);
            f32x4 a;
#pragma unroll
            for (int u = 0; u < 4; ++u) a[u] = ingest_one(r[u], bl, ratio, scale, clip01);
            *reinterpret_cast<f32x4*>(out + i) = a;
        }
    }
}

__global__ __launch_bounds__(RAWIO_T) void raw_emit_kernel(const float* __restrict__ x, size_t n, size_t head, size_t nvec, float bl, float scale,
                                                           float ratio, int undo_gain, uint16_t* __restrict__ out,
                                                           unsigned long long* __restrict__ n_saturated) {
    __shared__ int s_bad[RAWIO_T / 64];
    int bad = 0;
    if (blockIdx.x == 0 && threadIdx.x < 16) {
        const size_t tail0 = head + nvec * 8;
        const size_t i = threadIdx.x < 8 ? (size_t)threadIdx.x : tail0 + (threadIdx.x - 8);
        const bool mine = threadIdx.x < 8 ? (size_t)threadIdx.x < head : i < n;
        if (mine) out[i] = emit_one(x[i], bl, scale, ratio, undo_gain, bad);
    }
    const size_t step = (size_t)gridDim.x * RAWIO_T;
    for (size_t q = (size_t)blockIdx.x * RAWIO_T + threadIdx.x; q < nvec; q += step) {
        const size_t i = head + q * 8;
        float v[8];
        load8(x + i, v);
        u16x8 o;
#pragma unroll
        for (int u = 0; u < 8; ++u) o[u] = emit_one(v[u], bl, scale, ratio, undo_gain, bad);
        *reinterpret_cast<u16x8*>(out + i) = o;
    }
    if (n_saturated) {                                              // one wave reduction, one atomic per workgroup
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o);
        if ((threadIdx.x & 63) == 0) s_bad[threadIdx.x >> 6] = bad;
        __syncthreads();
        if (threadIdx.x == 0) {
            int t = 0;
#pragma unroll
            for (int w = 0; w < RAWIO_T / 64; ++w) t += s_bad[w];
            if (t) atomicAdd(n_saturated, (unsigned long long)t);
        }
    }
}

// elements in front of the first 16-byte boundary of `p` (element size es; p is element-aligned), at most n
static inline size_t rawio_head(const void* p, size_t es, size_t n) {
    const size_t off = (size_t)((uintptr_t)p & 15u);
    const size_t h = off ? (16 - off) / es : 0;
    return h < n ? h : n;
}

static inline unsigned rawio_grid(size_t nvec) {
    const size_t b = (nvec + RAWIO_T - 1) / RAWIO_T;
    return (unsigned)(b < 1 ? 1 : (b > RAWIO_MAX_BLOCKS ? RAWIO_MAX_BLOCKS : b));
}

template <typename T, int V>
static int raw_ingest(const T* raw, size_t n, float bl, float ratio, float scale, int clip01, float* out, void* stream) {
    if (!raw || !out || n == 0) return YOND_EINVAL;
    if (((uintptr_t)raw % sizeof(T)) || ((uintptr_t)out % sizeof(float))) return YOND_EINVAL;
    const size_t head = rawio_head(out, sizeof(float), n), nvec = (n - head) / V;
    hipLaunchKernelGGL((raw_ingest_kernel<T, V>), dim3(rawio_grid(nvec)), dim3(RAWIO_T), 0, (hipStream_t)stream, raw, n, head, nvec, bl, ratio,
                       scale, clip01, out);
    YOND_LAUNCH_CHECK();
    return YOND_OK;
}

extern "C" int yond_raw_ingest_u16(const uint16_t* raw, size_t n, float bl, float ratio, float scale, int clip01, float* out, void* stream) {
    return raw_ingest<uint16_t, 8>(raw, n, bl, ratio, scale, clip01, out, stream);
}

extern "C" int yond_raw_ingest_f32(const float* raw, size_t n, float bl, float ratio, float scale, int clip01, float* out, void* stream) {
    return raw_ingest<float, 4>(raw, n, bl, ratio, scale, clip01, out, stream);
}

extern "C" int yond_raw_emit_u16(const float* x, size_t n, float bl, float scale, float ratio, int undo_gain, uint16_t* out,
                                 unsigned long long* n_saturated, void* stream) {
    if (!x || !out || n == 0) return YOND_EINVAL;
    if (((uintptr_t)x % sizeof(float)) || ((uintptr_t)out % sizeof(uint16_t)) || ((uintptr_t)n_saturated % sizeof(unsigned long long)))
        return YOND_EINVAL;
    const size_t head = rawio_head(out, sizeof(uint16_t), n), nvec = (n - head) / 8;
    hipLaunchKernelGGL(raw_emit_kernel, dim3(rawio_grid(nvec)), dim3(RAWIO_T), 0, (hipStream_t)stream, x, n, head, nvec, bl, scale, ratio,
                       undo_gain, out, n_saturated);
    YOND_LAUNCH_CHECK();
    return YOND_OK;
}
