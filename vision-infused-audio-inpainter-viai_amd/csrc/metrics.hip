// Inpainting quality metrics on the device (gfx950): the sums behind SNR / SI-SDR over a gap in samples, L1 / PSNR / log-spectral distance over mel
// frames selected by the time mask, and the SSIM of two mel images.  Contracts: include/viai_hip.h, definitions and measured times: DESIGN.md 11.2k.
//
// Everything accumulates in fp64 from fp32 inputs, in a FIXED order: a thread sums its own elements in index order, a wave sums its lanes by the
// xor butterfly, a block sums its waves in wave order, and a second launch sums a stream's block partials in chunk order.  No atomics, and no kernel
// waits on another block: the second kernel is an ordinary launch behind the first on the same stream.  The chunks of a stream are laid over that
// stream's own region only (the gap from its first sample, the clip's frames, the clip's valid window positions), so a stream's numbers do not
// depend on which batch it is part of.
#include "viai_common.h"
#include "viai_internal.h"

namespace {

constexpr int MT_THREADS = 256;
constexpr int WG_CHUNK = 2048;        // samples of a gap per block: 8 per thread
constexpr int MF_FRAMES = 64;         // frames per block, one per lane; the block's four waves split the mel bands
constexpr int SS_TF = 16, SS_TT = 32; // SSIM: window positions per block, (mel band, frame)
constexpr int SS_MAX_TAPS = 31;

struct ss_window { double w[SS_MAX_TAPS]; };

// sum of K values over the block, the same bits in every thread of wave 0; every thread of the block calls it.  red: 4 * K doubles of LDS.
template <int K>
__device__ __forceinline__ void mt_block_sum(double (&v)[K], double* red) {
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = wave_sum_d(v[k]);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) red[wave * K + k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = ((red[k] + red[K + k]) + red[2 * K + k]) + red[3 * K + k];
}

// the gap of a stream clamped to the clip: [lo, hi) with 0 <= lo <= hi <= n
__device__ __forceinline__ void wg_bounds(int g0, int glen, int n, long* lo, long* hi) {
    long a = g0 < 0 ? 0 : g0;
    long b = (long)g0 + (glen < 0 ? 0 : glen);
    if (a > n) a = n;
    if (b > n) b = n;
    if (b < a) b = a;
    *lo = a;
    *hi = b;
}

// ---- wave: block (b, k) sums chunk k of stream b's gap, [lo + k C, lo + (k + 1) C) cut at hi, into ws[b][k][0..4) = {ref^2, est^2, err^2, ref est}
__global__ __launch_bounds__(MT_THREADS) void wave_gap_partial_kernel(const float* __restrict__ ref, const float* __restrict__ est,
                                                                      const int* __restrict__ g0, const int* __restrict__ glen,
                                                                      double* __restrict__ ws, int n, int nchunk) {
    __shared__ double red[16];
    const int b = blockIdx.x / nchunk, k = blockIdx.x - b * nchunk;
    long lo, hi;
    wg_bounds(g0[b], glen[b], n, &lo, &hi);
    const long c0 = lo + (long)k * WG_CHUNK;
    if (c0 >= hi) return;                                            // the whole block: the second pass reads the chunks below ceil(len / C) only
    const long c1 = c0 + WG_CHUNK < hi ? c0 + WG_CHUNK : hi;
    const float* __restrict__ r = ref + (long)b * n;
    const float* __restrict__ e = est + (long)b * n;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 8
    for (long i = c0 + threadIdx.x; i < c1; i += MT_THREADS) {
        const double x = (double)r[i], y = (double)e[i], d = x - y;
        s[0] += x * x;
        s[1] += y * y;
        s[2] += d * d;
        s[3] += x * y;
    }
    mt_block_sum<4>(s, red);
    if (threadIdx.x < 4) ws[((long)b * nchunk + k) * 4 + threadIdx.x] = s[threadIdx.x];
}

// ---- second pass of every metric: one wave per stream sums its K-wide partials in chunk order (lane l takes chunks l, l + 64, ...), then writes
// out[b][0] = count and out[b][1 .. K]; COUNT_IS_LEN: the count is the gap's clamped length and the partials hold K sums, else partial 0 is the count
template <int K, bool COUNT_IS_LEN>
__global__ __launch_bounds__(64) void mt_final_kernel(const double* __restrict__ ws, const int* __restrict__ g0, const int* __restrict__ glen,
                                                      double* __restrict__ out, int n, int nchunk) {
    const int b = blockIdx.x;
    int used = nchunk;
    long len = 0;
    if (COUNT_IS_LEN) {
        long lo, hi;
        wg_bounds(g0[b], glen[b], n, &lo, &hi);
        len = hi - lo;
        used = (int)((len + WG_CHUNK - 1) / WG_CHUNK);
    }
    double s[K];
#pragma unroll
    for (int j = 0; j < K; ++j) s[j] = 0.0;
    for (int k = threadIdx.x; k < used; k += 64) {
#pragma unroll
        for (int j = 0; j < K; ++j) s[j] += ws[((long)b * nchunk + k) * K + j];
    }
#pragma unroll
    for (int j = 0; j < K; ++j) s[j] = wave_sum_d(s[j]);
    if (threadIdx.x == 0) {
        if (COUNT_IS_LEN) {
            out[(long)b * (K + 1)] = (double)len;
#pragma unroll
            for (int j = 0; j < K; ++j) out[(long)b * (K + 1) + 1 + j] = s[j];
        } else {
#pragma unroll
            for (int j = 0; j < K; ++j) out[(long)b * K + j] = s[j];
        }
    }
}

// where: 0 every frame, 1 frames with mask == 0, 2 frames with mask != 0 (mask may be null for 0 only)
__device__ __forceinline__ bool mt_counts(const float* __restrict__ mask, long b, int T, int t, int where) {
    if (where == 0) return true;
    const bool known = mask[b * T + t] != 0.f;
    return where == 2 ? known : !known;
}

// ---- mel frames: block (b, k) takes frames [64 k, 64 k + 64); lane = frame (loads run along t), wave w sums the bands f = w, w + 4, ...
// ws[b][k][0..4) = {frames counted, sum |d|, sum d^2, sum_t db sqrt(mean_f d^2)}
__global__ __launch_bounds__(MT_THREADS) void mel_frame_partial_kernel(const float* __restrict__ ref, const float* __restrict__ est,
                                                                       const float* __restrict__ mask, double* __restrict__ ws, int F, int T,
                                                                       int nchunk, int where, double db_range) {
    __shared__ double band[4][MF_FRAMES][2];
    __shared__ double red[16];
    const int b = blockIdx.x / nchunk, k = blockIdx.x - b * nchunk;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int t = k * MF_FRAMES + lane;
    const float* __restrict__ r = ref + (long)b * F * T;
    const float* __restrict__ e = est + (long)b * F * T;
    const bool counted = t < T && mt_counts(mask, b, T, t, where);    // the same in the four waves; a frame that is not counted is not read
    double a1 = 0.0, a2 = 0.0;
    if (counted) {
#pragma unroll 4
        for (int f = wave; f < F; f += 4) {
            const double d = (double)e[(long)f * T + t] - (double)r[(long)f * T + t];
            a1 += fabs(d);
            a2 += d * d;
        }
    }
    band[wave][lane][0] = a1;
    band[wave][lane][1] = a2;
    __syncthreads();
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    if (wave == 0 && counted) {
        const double l1 = ((band[0][lane][0] + band[1][lane][0]) + band[2][lane][0]) + band[3][lane][0];
        const double l2 = ((band[0][lane][1] + band[1][lane][1]) + band[2][lane][1]) + band[3][lane][1];
        s[0] = 1.0;
        s[1] = l1;
        s[2] = l2;
        s[3] = db_range * sqrt(l2 / (double)F);
    }
    mt_block_sum<4>(s, red);
    if (threadIdx.x < 4) ws[((long)b * nchunk + k) * 4 + threadIdx.x] = s[threadIdx.x];
}

// ---- SSIM: block (b, tile) takes the 16 x 32 window positions from (f0, t0); position (f, t) reads the taps x taps pixels from (f, t) on and
// belongs to the frame of its centre, t + taps / 2.  The pixels of the tile and its halo are staged in LDS as doubles, zeros outside the image
// (positions that would read them are not counted); then, one moment plane at a time (x, y, x^2, y^2, x y), the row pass (along t) goes through
// LDS and the column pass (along f) into registers.  LDS: [ x | y | plane | window ], rows = 16 + taps - 1, cols = 32 + taps - 1.
// ws[b][tile][0..2) = {positions counted, sum of ssim}
__global__ __launch_bounds__(MT_THREADS) void mel_ssim_partial_kernel(const float* __restrict__ ref, const float* __restrict__ est,
                                                                      const float* __restrict__ mask, double* __restrict__ ws, int F, int T, int taps,
                                                                      int tiles_t, int ntile, int where, double c1, double c2, ss_window win) {
    extern __shared__ double lds[];
    const int rows = SS_TF + taps - 1, cols = SS_TT + taps - 1;
    double* __restrict__ sx = lds;
    double* __restrict__ sy = sx + rows * cols;
    double* __restrict__ plane = sy + rows * cols;                   // rows x 32
    double* __restrict__ sw = plane + rows * SS_TT;                  // 32 doubles (taps used); the reduction's 8 behind them
    double* __restrict__ red = sw + 32;
    const int b = blockIdx.x / ntile, tile = blockIdx.x - b * ntile;
    const int f0 = (tile / tiles_t) * SS_TF, t0 = (tile % tiles_t) * SS_TT;
    const float* __restrict__ r = ref + (long)b * F * T;
    const float* __restrict__ e = est + (long)b * F * T;
    const int PF = F - taps + 1, PT = T - taps + 1;
    const int tt = threadIdx.x & 31, fq = threadIdx.x >> 5;          // column pass: positions (fq, tt) and (fq + 8, tt) of the tile
    const bool counted = t0 + tt < PT && mt_counts(mask, b, T, t0 + tt + taps / 2, where);
    if (!__syncthreads_or(counted)) {                                // no centre frame of the tile is selected: nothing is read
        if (threadIdx.x < 2) ws[((long)b * ntile + tile) * 2 + threadIdx.x] = 0.0;
        return;
    }
    if (threadIdx.x < taps) sw[threadIdx.x] = win.w[threadIdx.x];
    for (int i = threadIdx.x; i < rows * cols; i += MT_THREADS) {
        const int rr = i / cols, cc = i - rr * cols;
        const int f = f0 + rr, t = t0 + cc;
        const bool in = f < F && t < T;
        sx[i] = in ? (double)r[(long)f * T + t] : 0.0;
        sy[i] = in ? (double)e[(long)f * T + t] : 0.0;
    }
    __syncthreads();
    double m[5][2];
#pragma unroll
    for (int p = 0; p < 5; ++p) {
        for (int i = threadIdx.x; i < rows * SS_TT; i += MT_THREADS) {
            const int rr = i >> 5, cc = i & 31;
            const double* __restrict__ px = sx + rr * cols + cc;
            const double* __restrict__ py = sy + rr * cols + cc;
            double acc = 0.0;
            for (int j = 0; j < taps; ++j) {
                const double x = px[j], y = py[j];
                const double v = p == 0 ? x : p == 1 ? y : p == 2 ? x * x : p == 3 ? y * y : x * y;
                acc += sw[j] * v;
            }
            plane[i] = acc;
        }
        __syncthreads();
        double u0 = 0.0, u1 = 0.0;
        for (int j = 0; j < taps; ++j) {
            u0 += sw[j] * plane[(fq + j) * SS_TT + tt];
            u1 += sw[j] * plane[(fq + 8 + j) * SS_TT + tt];
        }
        m[p][0] = u0;
        m[p][1] = u1;
        __syncthreads();                                             // the plane is rewritten by the next moment
    }
    double s[2] = {0.0, 0.0};
    if (counted) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (f0 + fq + 8 * h < PF) {
                const double mx = m[0][h], my = m[1][h];
                const double vx = m[2][h] - mx * mx, vy = m[3][h] - my * my, cxy = m[4][h] - mx * my;
                s[0] += 1.0;
                s[1] += ((2.0 * mx * my + c1) * (2.0 * cxy + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2));
            }
        }
    }
    mt_block_sum<2>(s, red);
    if (threadIdx.x < 2) ws[((long)b * ntile + tile) * 2 + threadIdx.x] = s[threadIdx.x];
}

inline long wg_chunks(int n) { return ((long)n + WG_CHUNK - 1) / WG_CHUNK; }
inline long mf_chunks(int T) { return ((long)T + MF_FRAMES - 1) / MF_FRAMES; }
inline long ss_tiles_f(int F, int taps) { return ((long)(F - taps + 1) + SS_TF - 1) / SS_TF; }
inline long ss_tiles_t(int T, int taps) { return ((long)(T - taps + 1) + SS_TT - 1) / SS_TT; }
inline bool ss_shape_ok(int F, int T, int taps) { return taps >= 1 && taps <= SS_MAX_TAPS && (taps & 1) == 1 && F >= taps && T >= taps; }
inline bool mt_grid_ok(long blocks) { return blocks >= 1 && blocks <= 0x7fffffffL; }
inline bool mt_f32_aligned(const void* p) { return ((uintptr_t)p & 3) == 0; }
inline bool mt_f64_aligned(const void* p) { return ((uintptr_t)p & 7) == 0; }

}  // namespace

extern "C" long viai_metrics_ws_doubles(int kind, int B, int n_or_F, int T, int taps) {
    if (B < 1 || n_or_F < 1) return 0;
    long per = 0;
    if (kind == VIAI_METRIC_WAVE) per = 4 * wg_chunks(n_or_F);
    else if (kind == VIAI_METRIC_MEL_FRAMES && T >= 1) per = 4 * mf_chunks(T);
    else if (kind == VIAI_METRIC_MEL_SSIM && ss_shape_ok(n_or_F, T, taps)) per = 2 * ss_tiles_f(n_or_F, taps) * ss_tiles_t(T, taps);
    return per > 0 && mt_grid_ok((long)B * per) ? (long)B * per : 0;
}

extern "C" int viai_wave_gap_stats(const float* ref, const float* est, const int* g0, const int* glen, double* out, double* ws, int B, int n,
                                   void* stream) {
    if (B < 1 || n < 1 || ref == nullptr || est == nullptr || g0 == nullptr || glen == nullptr || out == nullptr || ws == nullptr ||
        !mt_f32_aligned(ref) || !mt_f32_aligned(est) || !mt_f64_aligned(out) || !mt_f64_aligned(ws))
        return (int)hipErrorInvalidValue;
    const long nchunk = wg_chunks(n);
    if (!mt_grid_ok((long)B * nchunk)) return (int)hipErrorInvalidValue;
    VIAI_LAUNCH(wave_gap_partial_kernel, dim3((unsigned)(B * nchunk)), dim3(MT_THREADS), 0, (hipStream_t)stream, ref, est, g0, glen, ws, n, (int)nchunk);
    VIAI_LAUNCH((mt_final_kernel<4, true>), dim3(B), dim3(64), 0, (hipStream_t)stream, ws, g0, glen, out, n, (int)nchunk);
    return viai_launch_status();
}

extern "C" int viai_mel_frame_stats(const float* ref, const float* est, const float* mask, double* out, double* ws, int B, int F, int T, int where,
                                    double db_range, void* stream) {
    if (B < 1 || F < 1 || T < 1 || ref == nullptr || est == nullptr || out == nullptr || ws == nullptr || where < 0 || where > 2 ||
        (mask == nullptr && where != 0) || !mt_f32_aligned(ref) || !mt_f32_aligned(est) || !mt_f32_aligned(mask) || !mt_f64_aligned(out) ||
        !mt_f64_aligned(ws))
        return (int)hipErrorInvalidValue;
    const long nchunk = mf_chunks(T);
    if (!mt_grid_ok((long)B * nchunk) || (long)F * T > 0x7fffffffL) return (int)hipErrorInvalidValue;
    VIAI_LAUNCH(mel_frame_partial_kernel, dim3((unsigned)(B * nchunk)), dim3(MT_THREADS), 0, (hipStream_t)stream, ref, est, mask, ws, F, T, (int)nchunk,
                where, db_range);
    VIAI_LAUNCH((mt_final_kernel<4, false>), dim3(B), dim3(64), 0, (hipStream_t)stream, ws, (const int*)nullptr, (const int*)nullptr, out, 0,
                (int)nchunk);
    return viai_launch_status();
}

extern "C" int viai_mel_ssim(const float* ref, const float* est, const float* mask, const double* win, double* out, double* ws, int B, int F, int T,
                             int taps, int where, double c1, double c2, void* stream) {
    if (B < 1 || F < 1 || T < 1 || !ss_shape_ok(F, T, taps) || ref == nullptr || est == nullptr || win == nullptr || out == nullptr || ws == nullptr ||
        where < 0 || where > 2 || (mask == nullptr && where != 0) || !mt_f32_aligned(ref) || !mt_f32_aligned(est) || !mt_f32_aligned(mask) ||
        !mt_f64_aligned(win) || !mt_f64_aligned(out) || !mt_f64_aligned(ws))
        return (int)hipErrorInvalidValue;
    const long tiles_t = ss_tiles_t(T, taps), ntile = ss_tiles_f(F, taps) * tiles_t;
    if (!mt_grid_ok((long)B * ntile) || (long)F * T > 0x7fffffffL) return (int)hipErrorInvalidValue;
    ss_window w;
    for (int j = 0; j < SS_MAX_TAPS; ++j) w.w[j] = j < taps ? win[j] : 0.0;
    const int rows = SS_TF + taps - 1, cols = SS_TT + taps - 1;
    const size_t lds = sizeof(double) * (size_t)(2 * rows * cols + rows * SS_TT + 32 + 8);        // 24 KB at 11 taps, 58 KB at 31
    VIAI_LAUNCH(mel_ssim_partial_kernel, dim3((unsigned)(B * ntile)), dim3(MT_THREADS), lds, (hipStream_t)stream, ref, est, mask, ws, F, T, taps,
                (int)tiles_t, (int)ntile, where, c1, c2, w);
    VIAI_LAUNCH((mt_final_kernel<2, false>), dim3(B), dim3(64), 0, (hipStream_t)stream, ws, (const int*)nullptr, (const int*)nullptr, out, 0, (int)ntile);
    return viai_launch_status();
}
