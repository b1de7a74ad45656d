// Vocoder data preparation (gfx950): `_process_utterance` of utils/librivox.py:44-117 behind the file decode.  Contracts: include/viai_hip.h,
// derivation and figures: DESIGN.md 11.2h.  Two entry points, one launch each, every chunk of a file in that launch:
//     viai_utt_trim_bounds   the silence trim (utils/audio.py:56-67): first / last sample whose mu-law class leaves the silence band.  The class is
//                            computed on the fly by the device function viai_mulaw_quantize uses (viai_mulaw.h); no class array is written.
//     viai_utt_pack          the trimmed, rescaled waveform as an aligned row for the mel front end, and the training signal on the lws frame grid.
// Rescaling is x / amax * rescaling_max as numpy evaluates it on a float32 array: an IEEE division, then a multiplication, each rounded on its own
// (no reciprocal, nothing to contract; the Makefile has no fast-math flag and hipcc's fp32 division is the correctly rounded one by default).
// No LDS beyond the reduction slots, no atomics of any kind: a chunk's bounds are found by ONE block, so they do not depend on any order.
#include <climits>

#include "viai_common.h"
#include "viai_internal.h"
#include "viai_mulaw.h"

namespace {

constexpr int UT_NT = 1024;                  // threads of a trim block = samples of one scan step

__device__ __forceinline__ float utt_rescale(float x, bool rs, float amax, float rmax) { return rs ? x / amax * rmax : x; }

// min / max of one int per thread, handed to every thread of the block (blocks of UT_NT threads; all threads call)
__device__ __forceinline__ int utt_block_min(int v, int* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    int r = red[0];
#pragma unroll
    for (int w = 1; w < UT_NT / 64; ++w) r = min(r, red[w]);
    __syncthreads();                         // red is written again by the next step
    return r;
}
__device__ __forceinline__ int utt_block_max(int v, int* red) { return -utt_block_min(-v, red); }       // |v| < INT_MAX here

// the part of chunk c that lies inside the file: offset and clipped length (0 when the chunk does not start inside it)
__device__ __forceinline__ int utt_chunk(const int* __restrict__ off, const int* __restrict__ len, int c, long n, long* o) {
    const long oo = off[c];
    long L = len[c];
    if (oo < 0 || oo >= n || L < 0) L = 0;
    else if (oo + L > n) L = n - oo;
    *o = oo;
    return (int)L;
}

// One block per chunk.  The forward scan stops at the first step of UT_NT samples that holds an active one, the backward scan likewise from the end and
// never below max(2, start): speech costs two steps per chunk, a silent chunk is read once.  bounds[c] = (start, end), sentinels (len[c], -1).
__global__ __launch_bounds__(UT_NT) void utt_trim_bounds_kernel(const float* __restrict__ wav, long n, const int* __restrict__ off, const int* __restrict__ len,
                                                                const float* __restrict__ amax, float rmax, float mu, int thr, int sil, int* __restrict__ bounds) {
    __shared__ int red[UT_NT / 64];
    const int c = blockIdx.x, tid = threadIdx.x;
    long o;
    const int L = utt_chunk(off, len, c, n, &o);
    const float* y = wav + (L > 0 ? o : 0);
    const bool rs = amax != nullptr;
    const float am = rs ? *amax : 1.f;
    const float l1p = log1pf(mu);
    auto active = [&](int i) {
        const int k = viai_mulaw_class(utt_rescale(y[i], rs, am, rmax), mu, l1p);
        return abs(k - sil) > thr;
    };
    int start = len[c];
    bool found = false;
    for (int base = 0; base < L; base += UT_NT) {                                   // (uniform: L and the reduced value are the block's)
        const int i = base + tid;
        const int cand = utt_block_min((i < L && active(i)) ? i : INT_MAX, red);
        if (cand != INT_MAX) { start = cand; found = true; break; }
    }
    int end = -1;
    if (found) {
        const int lo = start > 2 ? start : 2;                                       // the reference's backward loop is range(size - 1, 1, -1)
        for (int top = L - 1; top >= lo; top -= UT_NT) {
            const int i = top - tid;
            const int cand = utt_block_max((i >= lo && active(i)) ? i : -1, red);
            if (cand >= 0) { end = cand; break; }
        }
    }
    if (tid == 0) { bounds[2 * c] = start; bounds[2 * c + 1] = end; }
}

__device__ __forceinline__ long utt_floordiv(long a, long b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// Items of a chunk: groups of four words, first the row's, then the signal's.  A full group whose destination is 16-byte aligned goes out as one
// vector store; the row's tail, the signal's tail and every group of a misaligned destination go out word by word.  Sources are scalar dword loads
// (the chunk start and the trim are arbitrary): a wave's four loads cover 1 KB of consecutive samples.
__global__ __launch_bounds__(256) void utt_pack_kernel(const float* __restrict__ wav, long n, const int* __restrict__ off, const int* __restrict__ len,
                                                       const int* __restrict__ bounds, const float* __restrict__ amax, float rmax, int mode, float mu,
                                                       int fft, int hop, const int* __restrict__ row_off, float* __restrict__ rows, long rows_cap,
                                                       const int* __restrict__ sig_off, unsigned* __restrict__ sig, long sig_cap, int vec_ok) {
    const int c = blockIdx.y;
    long o;
    const int L = utt_chunk(off, len, c, n, &o);
    int s = bounds[2 * c], e = bounds[2 * c + 1];
    s = s < 0 ? 0 : s;
    e = e > L ? L : e;
    if (e <= s) return;                                                             // nothing to write (the host refuses such a chunk before the launch)
    const int T = e - s;
    const long ro = row_off[c], so = sig_off[c];
    if (ro < 0 || so < 0) return;
    const float* y = wav + o + s;
    const int lp = fft - hop;
    const long S = (utt_floordiv((long)T + 2L * lp - fft, hop) + (T % hop == 0 ? 1 : 2)) * hop;      // lws_num_frames(T) * hop
    const bool rs = amax != nullptr;
    const float am = rs ? *amax : 1.f;
    const float l1p = log1pf(mu);
    const unsigned pad = mode == VIAI_UTT_MULAW_QUANTIZE ? (unsigned)((int)mu / 2) : 0u;
    const long g_row = ((long)T + 3) / 4, g_sig = (S + 3) / 4;
    for (long g = blockIdx.x * 256L + threadIdx.x; g < g_row + g_sig; g += (long)gridDim.x * 256L) {
        if (g < g_row) {
            const long i0 = 4 * g, d0 = ro + i0;
            float v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = i0 + k < T ? utt_rescale(y[i0 + k], rs, am, rmax) : 0.f;
            if (vec_ok && (ro & 3) == 0 && i0 + 4 <= T && d0 + 4 <= rows_cap) {
                *reinterpret_cast<f32x4*>(rows + d0) = f32x4{v[0], v[1], v[2], v[3]};
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (i0 + k < T && d0 + k < rows_cap) rows[d0 + k] = v[k];
            }
        } else {
            const long j0 = 4 * (g - g_row), d0 = so + j0;
            unsigned w[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const long i = j0 + k - lp;
                w[k] = pad;
                if (i >= 0 && i < T) {
                    const float x = utt_rescale(y[i], rs, am, rmax);
                    if (mode == VIAI_UTT_MULAW_QUANTIZE) w[k] = (unsigned)viai_mulaw_class(x, mu, l1p);
                    else if (mode == VIAI_UTT_MULAW) w[k] = __float_as_uint(viai_mulaw_compand(x, mu, l1p));
                    else w[k] = __float_as_uint(x);
                }
            }
            if (vec_ok && (so & 3) == 0 && j0 + 4 <= S && d0 + 4 <= sig_cap) {
                *reinterpret_cast<u32x4*>(sig + d0) = u32x4{w[0], w[1], w[2], w[3]};
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (j0 + k < S && d0 + k < sig_cap) sig[d0 + k] = w[k];
            }
        }
    }
}

inline bool utt_mode_ok(int mode) { return mode == VIAI_UTT_MULAW_QUANTIZE || mode == VIAI_UTT_MULAW || mode == VIAI_UTT_RAW; }

}  // namespace

extern "C" int viai_utt_trim_bounds(const float* wav, long n_samples, const int* chunk_off, const int* chunk_len, int n_chunks, const float* amax,
                                    float rescaling_max, int mu, int thr, int silence_class, int* bounds, void* stream) {
    if (wav == nullptr || chunk_off == nullptr || chunk_len == nullptr || bounds == nullptr || n_chunks < 1 || n_samples < 1 || n_samples > (long)INT_MAX ||
        mu < 1 || thr < 0)
        return (int)hipErrorInvalidValue;
    VIAI_LAUNCH(utt_trim_bounds_kernel, dim3(n_chunks), dim3(UT_NT), 0, (hipStream_t)stream, wav, n_samples, chunk_off, chunk_len, amax, rescaling_max,
                (float)mu, thr, silence_class, bounds);
    return viai_launch_status();
}

extern "C" int viai_utt_pack(const float* wav, long n_samples, const int* chunk_off, const int* chunk_len, const int* bounds, int n_chunks, int max_len,
                             const float* amax, float rescaling_max, int mode, int mu, int fft, int hop, const int* row_off, float* rows, long rows_cap,
                             const int* sig_off, void* signal, long signal_cap, void* stream) {
    if (wav == nullptr || chunk_off == nullptr || chunk_len == nullptr || bounds == nullptr || row_off == nullptr || rows == nullptr || sig_off == nullptr ||
        signal == nullptr || n_chunks < 1 || n_chunks > 65535 || max_len < 1 || n_samples < 1 || n_samples > (long)INT_MAX || rows_cap < 1 ||
        rows_cap > (long)INT_MAX || signal_cap < 1 || signal_cap > (long)INT_MAX || mu < 1 || fft < 1 || hop < 1 || hop > fft || !utt_mode_ok(mode) ||
        ((uintptr_t)rows & 3) != 0 || ((uintptr_t)signal & 3) != 0)
        return (int)hipErrorInvalidValue;
    const int vec_ok = ((uintptr_t)rows & 15) == 0 && ((uintptr_t)signal & 15) == 0;
    long gx = ((2L * max_len + fft + hop) / 4 + 255) / 256;                        // the grid's width only: the kernel strides over whatever a chunk holds
    gx = gx < 1 ? 1 : (gx > 256 ? 256 : gx);
    VIAI_LAUNCH(utt_pack_kernel, dim3((unsigned)gx, (unsigned)n_chunks), dim3(256), 0, (hipStream_t)stream, wav, n_samples, chunk_off, chunk_len, bounds, amax,
                rescaling_max, mode, (float)mu, fft, hop, row_off, rows, rows_cap, sig_off, reinterpret_cast<unsigned*>(signal), signal_cap, vec_ok);
    return viai_launch_status();
}
