// Rational-ratio polyphase resampler (gfx950): a waveform at sr_in comes out at sr_out = sr_in L / M.  Contracts: include/viai_hip.h, formula, layout
// and measured rates: DESIGN.md 11.2l.
//
// Host side: the plan (L, M, H, T), the Kaiser-windowed sinc table in fp64 rounded once to fp32, the output length, and the widening of a gap by
// the filter's support (viai_gap_at_rate, the resampler's counterpart of gap_frames).  None of it touches the device.
//
// Device side, one launch for a batch: output k of a row is sum_j x[i0 - H + j] * h[j][q], q = k mod L, i0 = (k / L) M + first[q].  The table is in
// PERIOD ORDER and tap-major (h[j * L + q]), so the threads of a wave, which take consecutive q, read consecutive words of it.  A block owns a tile
// of consecutive outputs of one row and stages the contiguous input span they read in LDS (zeros outside [0, length)).  A thread takes PP outputs
// with the SAME q, PP periods apart, so one table word feeds PP accumulators: the table stays in L2 / L1 and is read once per PP outputs.
// Every output is one chain acc = fmaf(x, h, acc), j = 0 .. T - 1, from +0: the bits of y[k] depend on the row's samples and the table alone, not
// on the batch, the tile, the launch geometry or the window.
#include <cmath>
#include <vector>

#include "viai_common.h"
#include "viai_internal.h"

namespace {

constexpr int WR_THREADS = 256;
constexpr int WR_PP = 4;                       // outputs per work item in the period form
constexpr long WR_MAX_TABLE = 1L << 22;        // L * T words: 16 MiB (VIAI_WAV_RESAMPLE_MAX_TABLE)
constexpr long WR_MAX_SPAN = 16384;            // words of LDS a block may stage: 64 KiB
constexpr int WR_PERIOD_MAX_L = 512;           // above it a period is longer than a tile is worth: the consecutive form

// A tile is `lt * g * PP` consecutive outputs starting at a multiple of that; work item w of a tile, pass pp, is output
//     k = tile_start + ((w / lt) + g * pp) * lt + (w % lt),          w in [0, lt * g).
// Period form: lt = L, PP = 4 (item w keeps q = w % L and takes periods w / L, w / L + g, ...: consecutive lanes take consecutive q).
// Consecutive form: PP = 1, g = 1, lt = the tile itself.
template <int PP>
__global__ __launch_bounds__(WR_THREADS) void wav_resample_kernel(const float* __restrict__ x, const int* __restrict__ lengths,
                                                                  const float* __restrict__ taps, const int* __restrict__ first,
                                                                  float* __restrict__ y, const int* __restrict__ o0, const int* __restrict__ o1,
                                                                  long x_stride, long y_stride, int m, int L, int M, int H, int T, int lt, int g,
                                                                  int ntiles, int span) {
    extern __shared__ __align__(16) float xs[];
    const int b = blockIdx.x / ntiles, tile = blockIdx.x - b * ntiles;
    const int items = lt * g;
    const long tile_len = (long)items * PP;
    const long k_start = (long)tile * tile_len;
    long w0 = o0 != nullptr ? (long)o0[b] : 0, w1 = o1 != nullptr ? (long)o1[b] : (long)m;
    if (w0 < 0) w0 = 0;
    if (w1 > m) w1 = m;
    if (k_start >= w1 || k_start + tile_len <= w0) return;               // the whole block: this tile holds no output of the window
    long len = lengths != nullptr ? (long)lengths[b] : x_stride;
    if (len < 0) len = 0;
    if (len > x_stride) len = x_stride;
    const long span_lo = k_start * M / L - H;                            // floor: k_start, M >= 0
    const float* __restrict__ xr = x + (long)b * x_stride;
    for (int s = threadIdx.x; s < span; s += WR_THREADS) {
        const long i = span_lo + s;
        xs[s] = (i >= 0 && i < len) ? xr[i] : 0.f;
    }
    __syncthreads();
    float* __restrict__ yr = y + (long)b * y_stride;
    for (int w = threadIdx.x; w < items; w += WR_THREADS) {
        const int wp = w / lt, wq = w - wp * lt;
        long k[PP];
        int base[PP];
        bool live[PP], any = false;
        unsigned q = 0;
#pragma unroll
        for (int pp = 0; pp < PP; ++pp) {
            k[pp] = k_start + (long)(wp + g * pp) * lt + wq;
            live[pp] = k[pp] >= w0 && k[pp] < w1;
            any = any || live[pp];
            const unsigned ku = (unsigned)k[pp];                           // k < tile_start + tile_len <= m + tile_len: fits 32 bits (checked by the host)
            const unsigned p = ku / (unsigned)L;
            q = ku - p * (unsigned)L;                                      // the same for every pp in the period form
            base[pp] = (int)((long)p * M + first[q] - H - span_lo);        // in [0, span - T]
        }
        if (!any) continue;
        float acc[PP];
#pragma unroll
        for (int pp = 0; pp < PP; ++pp) acc[pp] = 0.f;
        const float* __restrict__ hq = taps + q;
#pragma unroll 4
        for (int j = 0; j < T; ++j) {
            const float h = hq[(long)j * L];
#pragma unroll
            for (int pp = 0; pp < PP; ++pp) acc[pp] = fmaf(xs[base[pp] + j], h, acc[pp]);
        }
#pragma unroll
        for (int pp = 0; pp < PP; ++pp)
            if (live[pp]) yr[k[pp]] = acc[pp];
    }
}

inline long wr_gcd(long a, long b) {
    while (b != 0) {
        const long t = a % b;
        a = b;
        b = t;
    }
    return a;
}

inline long wr_floor_div(long a, long b) {                                // b > 0
    long q = a / b;
    if ((a % b != 0) && (a < 0)) --q;
    return q;
}
inline long wr_ceil_div(long a, long b) { return -wr_floor_div(-a, b); }   // b > 0

// words a tile of tile_len outputs stages: i0 moves by at most floor((tile_len - 1) M / L) + 1 inside it, and each output reads [i0 - H, i0 + H]
inline long wr_span(long tile_len, int L, int M, int H) { return (tile_len - 1) * M / L + 2L * H + 3; }

bool wr_geom(long sr_in, long sr_out, int zeros, int* L, int* M, int* H, int* T) {
    if (sr_in < 1 || sr_out < 1 || zeros < 1 || sr_in > 0x7fffffffL || sr_out > 0x7fffffffL) return false;
    const long g = wr_gcd(sr_in, sr_out);
    const long l = sr_out / g, mm = sr_in / g;
    const long h = mm > l ? wr_ceil_div((long)zeros * mm, l) : (long)zeros;   // ceil(zeros / min(1, L / M))
    const long t = 2 * h + 1;
    if (h > 0x3fffffffL || l * t > WR_MAX_TABLE) return false;
    *L = (int)l;
    *M = (int)mm;
    *H = (int)h;
    *T = (int)t;
    return true;
}

// modified Bessel function of the first kind, order 0: sum_k ((v / 2)^k / k!)^2, every term positive, until a term no longer changes the sum
double wr_i0(double v) {
    const double q = 0.25 * v * v;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 500; ++k) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < 1e-17 * sum) break;
    }
    return sum;
}

struct wr_launch { int pp, lt, g; long span; };

// the launch form of a plan; pp = 0: no tile of it fits the LDS budget
wr_launch wr_pick(int L, int M, int H) {
    wr_launch best = {0, 0, 0, 0};
    if (L <= WR_PERIOD_MAX_L) {
        // g periods per pass: the items L g are worked off in ceil(L g / 256) passes of the block, and the lanes of the last pass beyond L g idle.
        // Take g = 1 if its span fits, and a larger g only where it fills the passes' lanes better by more than a hundredth: among equally full
        // forms the smallest tile wins (more blocks).  Integers: items / slots > 1.01 best_items / best_slots.
        long best_items = 0, best_slots = 1;
        const int gmax = 1024 / L > 1 ? 1024 / L : 1;
        for (int g = 1; g <= gmax; ++g) {
            const long items = (long)L * g, span = wr_span(items * WR_PP, L, M, H);
            if (span > WR_MAX_SPAN) break;
            const long slots = ((items + WR_THREADS - 1) / WR_THREADS) * WR_THREADS;
            if (g == 1 || items * best_slots * 100 > best_items * slots * 101) {
                best_items = items;
                best_slots = slots;
                best = {WR_PP, L, g, span};
            }
        }
        if (best.pp != 0) return best;
    }
    for (int lt = 1024; lt >= 64; lt >>= 1) {
        const long span = wr_span(lt, L, M, H);
        if (span <= WR_MAX_SPAN) return {1, lt, 1, span};
    }
    return best;
}

}  // namespace

extern "C" int viai_wav_resample_geom(int sr_in, int sr_out, int zeros, int* L, int* M, int* H, int* T) {
    if (L == nullptr || M == nullptr || H == nullptr || T == nullptr) return (int)hipErrorInvalidValue;
    return wr_geom(sr_in, sr_out, zeros, L, M, H, T) ? 0 : (int)hipErrorInvalidValue;
}

extern "C" int viai_wav_resample_form(int L, int M, int H, int* pp, int* lt, int* g, int* span) {
    if (pp == nullptr || lt == nullptr || g == nullptr || span == nullptr || L < 1 || M < 1 || H < 0) return (int)hipErrorInvalidValue;
    const wr_launch f = wr_pick(L, M, H);
    *pp = f.pp;
    *lt = f.lt;
    *g = f.g;
    *span = (int)f.span;                                                 // at most WR_MAX_SPAN, 0 with pp = 0
    return 0;
}

extern "C" int viai_wav_resample_taps(int sr_in, int sr_out, int zeros, double rolloff, double beta, float* taps, int* first) {
    int L, M, H, T;
    if (taps == nullptr || first == nullptr || !wr_geom(sr_in, sr_out, zeros, &L, &M, &H, &T) || !(rolloff > 0.0) || !(rolloff <= 1.0) ||
        !(beta >= 0.0) || !(beta < 700.0))
        return (int)hipErrorInvalidValue;
    const double pi = 3.14159265358979323846;
    const double s = (double)L / (double)M < 1.0 ? (double)L / (double)M : 1.0;
    const double c = rolloff * s, W = (double)zeros / s, i0_beta = wr_i0(beta);
    for (int q = 0; q < L; ++q) {
        const long qm = (long)q * M;
        const long r = qm % L;
        first[q] = (int)(qm / L);
        for (int j = 0; j < T; ++j) {
            const double t = (double)r / (double)L - (double)(j - H);
            const double u = t / W;
            double h = 0.0;
            if (std::fabs(u) < 1.0) {
                const double v = pi * (c * t);                           // sinc(c t): where c t is an integer the tap is the rounding of pi v
                const double sinc = v == 0.0 ? 1.0 : std::sin(v) / v;
                h = c * sinc * wr_i0(beta * std::sqrt(1.0 - u * u)) / i0_beta;
            }
            taps[(long)j * L + q] = (float)h;
        }
    }
    return 0;
}

extern "C" long viai_wav_resample_out_len(long n, int L, int M) {
    if (n < 0 || L < 1 || M < 1) return 0;
    return (long)(((__int128)n * L + M - 1) / M);
}

extern "C" int viai_gap_at_rate(long g0, long g1, int L, int M, int H, long m, long* k0, long* k1) {
    if (k0 == nullptr || k1 == nullptr || L < 1 || M < 1 || H < 0 || m < 0) return (int)hipErrorInvalidValue;
    *k0 = 0;
    *k1 = 0;
    if (g1 <= g0) return 0;
    if (g0 < -(1L << 40) || g1 > (1L << 40)) return (int)hipErrorInvalidValue;      // (g + H) L stays far inside 64 bits
    long a = wr_ceil_div((g0 - H) * L, M), b = wr_ceil_div((g1 + H) * L, M);
    if (a < 0) a = 0;
    if (b > m) b = m;
    if (b > a) {
        *k0 = a;
        *k1 = b;
    }
    return 0;
}

extern "C" int viai_wav_resample(const float* x, const int* lengths, const float* taps, const int* first, float* y, const int* o0, const int* o1,
                                 int B, long x_stride, long y_stride, int m, int L, int M, int H, int T, void* stream) {
    if (x == nullptr || taps == nullptr || first == nullptr || y == nullptr || B < 1 || m < 1 || L < 1 || M < 1 || T < 1 || H < 0 ||
        (long)T != 2L * H + 1 || x_stride < 1 || y_stride < (long)m || (long)L * T > WR_MAX_TABLE || ((uintptr_t)x & 3) != 0 ||
        ((uintptr_t)y & 3) != 0 || ((uintptr_t)taps & 3) != 0)
        return (int)hipErrorInvalidValue;
    const wr_launch f = wr_pick(L, M, H);
    if (f.pp == 0) return (int)hipErrorInvalidValue;                     // 2 H + 3 words and one output's step do not fit 64 KiB of LDS
    const long tile_len = (long)f.lt * f.g * f.pp;
    const long ntiles = ((long)m + tile_len - 1) / tile_len;
    if (ntiles * tile_len > 0xffffffffL || (long)B * ntiles > 0x7fffffffL) return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)(B * ntiles)), block(WR_THREADS);
    const size_t lds = sizeof(float) * (size_t)f.span;
    if (f.pp == WR_PP)
        VIAI_LAUNCH(wav_resample_kernel<WR_PP>, grid, block, lds, (hipStream_t)stream, x, lengths, taps, first, y, o0, o1, x_stride, y_stride, m, L, M,
                    H, T, f.lt, f.g, (int)ntiles, (int)f.span);
    else
        VIAI_LAUNCH(wav_resample_kernel<1>, grid, block, lds, (hipStream_t)stream, x, lengths, taps, first, y, o0, o1, x_stride, y_stride, m, L, M, H, T,
                    f.lt, f.g, (int)ntiles, (int)f.span);
    return viai_launch_status();
}
