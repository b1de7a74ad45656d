// Dropout of the WaveNet residual layers (modules.py:173-175) with a counter-based mask (gfx950): y[i] = keep(i) ? x[i] * scale : +0.
// keep(i) is a pure function of (seed, offset, i) -- Philox4x32-10 (Salmon et al., SC'11; the Random123 constants), one call per four
// consecutive elements -- so the backward pass recomputes the mask from three integers and no mask tensor exists.  The same kernel
// serves both directions: d/dx of x * m * scale is the same map applied to dy.
#include "viai_common.h"
#include "viai_internal.h"

namespace {

// counter c, key (k0, k1) -> four 32-bit words.  The key schedule is uniform over the grid (scalar registers); a round is two
// 32 x 32 -> 64 bit products and four XORs per lane.
__device__ __forceinline__ u32x4 philox4x32_10(u32x4 c, unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = 0xD2511F53ull * c[0], p1 = 0xCD9E8D57ull * c[2];
        c = u32x4{(unsigned)(p1 >> 32) ^ c[1] ^ k0, (unsigned)p1, (unsigned)(p0 >> 32) ^ c[3] ^ k1, (unsigned)p0};
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c;
}

// the words of elements 4 j .. 4 j + 3: counter = (j lo, j hi, offset lo, offset hi), key = (seed lo, seed hi)
__device__ __forceinline__ u32x4 dropout_words(long j, unsigned o0, unsigned o1, unsigned k0, unsigned k1) {
    return philox4x32_10(u32x4{(unsigned)j, (unsigned)((unsigned long long)j >> 32), o0, o1}, k0, k1);
}

// x and y may be the same pointer (every element is read and written by the same lane, the load first): no __restrict__.
// A dropped element is a select of +0, never a product: inf / NaN inputs do not leak through a dropped position.
__global__ __launch_bounds__(256) void dropout_kernel(const float* x, float* y, long n, float scale, unsigned thr, unsigned k0, unsigned k1,
                                                      unsigned o0, unsigned o1) {
    const long n4 = n >> 2;
    const f32x4* x4 = reinterpret_cast<const f32x4*>(x);
    f32x4* y4 = reinterpret_cast<f32x4*>(y);
    for (long j = blockIdx.x * 256L + threadIdx.x; j < n4; j += (long)gridDim.x * 256L) {
        const f32x4 v = x4[j];                                          // issued first: the ten rounds run under the load
        const u32x4 w = dropout_words(j, o0, o1, k0, k1);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = w[e] >= thr ? v[e] * scale : 0.f;
        y4[j] = o;
    }
    // the last n % 4 elements: the same counter (j = n / 4) and word e for element 4 j + e, scalar accesses
    const int e = (int)threadIdx.x;
    if (blockIdx.x == 0 && e < (int)(n & 3)) {
        const u32x4 w = dropout_words(n4, o0, o1, k0, k1);
        const unsigned we = e == 0 ? w[0] : (e == 1 ? w[1] : w[2]);
        const float v = x[4 * n4 + e];
        y[4 * n4 + e] = we >= thr ? v * scale : 0.f;
    }
}

}  // namespace

extern "C" int viai_dropout(const float* x, float* y, long n, double p, unsigned long long seed, unsigned long long offset, void* stream) {
    if (!(p >= 0.0 && p < 1.0) || n < 0) return (int)hipErrorInvalidValue;                     // NaN fails the first comparison
    if (n == 0) return 0;
    if (n >= 4 && ((reinterpret_cast<size_t>(x) | reinterpret_cast<size_t>(y)) & 15)) return (int)hipErrorInvalidValue;   // 16-byte accesses
    const unsigned thr = (unsigned)__builtin_floor(p * 4294967296.0);                          // keep iff word >= thr: P(drop) = thr / 2^32
    const float scale = (float)(1.0 / (1.0 - p));                                              // rounded once
    // memory-bound streaming: at most 2048 blocks (8 per CU: 8 waves per SIMD, all resident at once), the rest by the grid stride
    long blocks = ((n >> 2) + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    VIAI_LAUNCH(dropout_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, y, n, scale, thr, (unsigned)seed,
                (unsigned)(seed >> 32), (unsigned)offset, (unsigned)(offset >> 32));
    return viai_launch_status();
}
