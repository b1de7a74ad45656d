// Where a waveform holds clicks (gfx950): impulsive damage found as outliers of a prediction residual, as the ordered (start, length) lists
// find_gaps writes.  Contract and rule: include/viai_hip.h; the arithmetic, with the order of every sum: viai_click_rule.h (on top of
// viai_ar_rule.h); launch shapes, LDS budget and serial depth: DESIGN.md 11.2r.
//
// Four launches for the batch, no atomics, nothing allocated, nothing synced:
//   1  cd_flag_kernel    one block of 256 threads per TILE of 4096 samples (the tiles of gap_detect.hip).  The tile goes into LDS as fp64 F and B
//                        and Burg's recursion runs on it stage by stage (ar_burg_block<1> of viai_ar_fit.h: one side of ar_fill_kernel).  Then
//                        thread t computes the residuals of its samples i = t, t + 256, ... -- 16 accumulators fed from one broadcast
//                        coefficient per step, the history read from global memory (the tile itself and the previous tile's tail: L2-hot) --
//                        and keeps their squares in registers: partial t of every variance sum is thread t's own, so the 1 + passes
//                        reductions are the fit's tree and nothing is stored in between.  The raw flags leave as wave64 ballots: wave w's
//                        k-th ballot is word w + 4 k of the tile, the mask layout of find_gaps.
//   2  cd_dilate_kernel  one wave per tile, lane = word.  Reads flag words w - 1, w, w + 1 of the ROW (so the dilation crosses words and tiles),
//                        widens by guard <= 64 on both sides, cuts at the row's length, and writes the final mask word and the tile's summary
//                        with the function gd_mask_kernel uses (gd_tile_summary).
//   3, 4  gd_rows_kernel, gd_emit_kernel of gap_detect.hip, unchanged (viai_gd_launch_runs).
// A flag is judged by the block that holds the sample; dilation works on bits alone, so no result depends on which block computes it.
#include <cmath>
#include <vector>

#include "viai_common.h"
#include "viai_gap_runs.h"
#include "viai_click_rule.h"
#include "viai_ar_fit.h"

#pragma clang fp contract(off)

namespace {

constexpr int CD_PER = GD_TILE / AR_THREADS;                               // samples of a tile per thread
constexpr int CD_LDS_DOUBLES = 2 * GD_TILE + ar_small_doubles(1) + 4 + 2;   // F, B, coef and red of the fit, 4 wave sums, 4 wave counts (ints)
static_assert(GD_THREADS == AR_THREADS && CD_PER * AR_THREADS == GD_TILE, "thread t owns the samples t, t + 256, ... of the tile");
static_assert(CD_PER * 4 == GD_WORDS, "wave w's k-th ballot is word w + 4 k");
static_assert(CD_LDS_DOUBLES * sizeof(double) <= 80 * 1024, "two blocks per CU");
static_assert(GD_TILE <= AR_MAX_CONTEXT, "a tile is a context of the fit");

__global__ __launch_bounds__(AR_THREADS) void cd_flag_kernel(const float* __restrict__ wav, const int* __restrict__ lengths, long stride, int n,
                                                             int ntiles, int order, double kk, double ff, int passes,
                                                             unsigned long long* __restrict__ flags) {
    extern __shared__ double lds[];
    const int b = blockIdx.x / ntiles, t = blockIdx.x - b * ntiles;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int len = gd_row_len(lengths, b, n);
    const int base = t * GD_TILE;                                           // < 2^31: ntiles GD_TILE <= 2^31 (checked by the host)
    const int left = len - base;
    const int C = left < GD_TILE ? (left > 0 ? left : 0) : GD_TILE;         // the tile's samples; none at or beyond len is read
    const int p = cd_order(order, C);
    const float* __restrict__ xr = wav + (long)b * stride;
    double* F = lds;
    double* coef = lds + 2 * GD_TILE;                                       // [buffer][AR_COEF]
    double* red = coef + 2 * AR_COEF;                                       // [wave][3]
    double* vred = red + 4 * 3;                                             // [wave]
    int* cred = reinterpret_cast<int*>(vred + 4);                           // [wave]

    float x[CD_PER];
#pragma unroll
    for (int k = 0; k < CD_PER; ++k) {
        const int i = tid + k * AR_THREADS;
        x[k] = i < C ? xr[base + i] : 0.f;
    }
    double q[CD_PER];
    bool judged[CD_PER];
    double var = 0.0;
#pragma unroll
    for (int k = 0; k < CD_PER; ++k) {
        q[k] = 0.0;
        judged[k] = false;
    }
    if (p >= 1) {                                                           // the whole block
        // 1  the fit
#pragma unroll
        for (int k = 0; k < CD_PER; ++k) {
            const int i = tid + k * AR_THREADS;
            if (i < C) {
                const double v = ar_sample(x[k]);
                F[i] = v;
                F[GD_TILE + i] = v;
            }
        }
        if (tid == 0) coef[0] = 1.0;
        __syncthreads();
        const long Cs[1] = {C};
        const int ps[1] = {p};
        int cur[1] = {0};
        ar_burg_block<1>(lds, 0L, (long)GD_TILE, Cs, ps, coef, red, cur);
        const double* a = coef + cur[0] * AR_COEF;
        // 2  the residuals: a[j] is one broadcast read per step, the 16 chains are independent
#pragma unroll
        for (int k = 0; k < CD_PER; ++k) {
            const int i = tid + k * AR_THREADS;
            judged[k] = i < C && base + i >= p;
        }
        for (int j = 0; j <= p; ++j) {
            const double aj = a[j];
#pragma unroll
            for (int k = 0; k < CD_PER; ++k) {
                const int i = tid + k * AR_THREADS;
                if (judged[k]) q[k] = ar_mac(q[k], aj, ar_sample(xr[base + i - j]));     // base + i - j >= p - j >= 0
            }
        }
#pragma unroll
        for (int k = 0; k < CD_PER; ++k) q[k] = q[k] * q[k];
        // 3  the scale: the mean of the squares, then of those under the cut
        for (int r = 0; r <= passes; ++r) {
            double s = 0.0;
            int c = 0;
#pragma unroll
            for (int k = 0; k < CD_PER; ++k) {
                if (judged[k] && (r == 0 || cd_keep(q[k], kk, var))) {
                    s = cd_add(s, q[k]);
                    c += 1;
                }
            }
            s = wave_sum_d_dpp(s);                                            // every lane of every wave is here
            c = gd_wave_all(c, OpAdd());
            if (lane == 0) {
                vred[wv] = s;
                cred[wv] = c;
            }
            __syncthreads();
            var = cd_mean(ar_sum4(vred[0], vred[1], vred[2], vred[3]), (long)(cred[0] + cred[1] + cred[2] + cred[3]), var);
            __syncthreads();
        }
    }
    // 4  the flags, one word per wave and k
    const long at = (long)b * ntiles + t;
#pragma unroll
    for (int k = 0; k < CD_PER; ++k) {
        const int i = tid + k * AR_THREADS;
        const bool f = i < C && (cd_nonfinite(x[k]) || (judged[k] && cd_flag(q[k], kk, var, ff)));
        const unsigned long long w = __ballot(f);
        if (lane == 0) flags[at * GD_WORDS + wv + 4 * k] = w;
    }
}

// bit i of the result: any bit of the 192-bit window (lo, mid, hi) within g of bit i of mid; 0 <= g <= 64
__device__ __forceinline__ unsigned long long cd_dilate_word(unsigned long long lo, unsigned long long mid, unsigned long long hi, int g) {
    unsigned long long r = mid;
    for (int d = 1; d <= g; ++d) {
        const unsigned long long up = d < 64 ? (mid << d) | (lo >> (64 - d)) : lo;      // bit i - d
        const unsigned long long dn = d < 64 ? (mid >> d) | (hi << (64 - d)) : hi;      // bit i + d
        r |= up | dn;
    }
    return r;
}

__global__ __launch_bounds__(GD_THREADS) void cd_dilate_kernel(const unsigned long long* __restrict__ flags, const int* __restrict__ lengths, int n,
                                                               int ntiles, int guard, int min_len, int mw, unsigned long long* __restrict__ mask,
                                                               int* __restrict__ tab, long tiles_total) {
    const int lane = threadIdx.x & 63;
    const long at = (long)blockIdx.x * GD_WAVES + (threadIdx.x >> 6);
    if (at >= tiles_total) return;                                          // whole waves from here on
    const int b = (int)(at / ntiles), t = (int)(at - (long)b * ntiles), base = t * GD_TILE;
    const int len = gd_row_len(lengths, b, n);
    const unsigned long long* __restrict__ fr = flags + (long)b * ntiles * GD_WORDS;    // the row's flag words
    const long nw = (long)ntiles * GD_WORDS;
    auto word = [&](long j) { return j >= 0 && j < nw ? fr[j] : 0ull; };
    const long w = (long)t * GD_WORDS + lane;
    unsigned long long m = cd_dilate_word(word(w - 1), word(w), word(w + 1), guard);
    const long room = (long)len - 64 * w;                                   // no flag lies at or beyond len; the dilation must not either
    m &= room >= 64 ? ~0ull : (room <= 0 ? 0ull : ((1ull << room) - 1ull));
    int hp = 0;                                                             // the final mask bit of the sample in front of the tile
    if (t > 0 && base - 1 < len) {
        const long pw = (long)t * GD_WORDS - 1;
        hp = (int)(cd_dilate_word(word(pw - 1), word(pw), word(pw + 1), guard) >> 63);
    }
    gd_tile_summary(m, hp, at, base, lane, min_len, mw, mask, tab, tiles_total);
}

inline bool cd_rule_ok(long stride, long n, int order, float k, int passes, int guard, float floor, int min_len, int merge_within) {
    return stride >= n && order >= 1 && order <= AR_MAX_ORDER && k > 0.f && k <= 3.402823466e38f && passes >= 0 && passes <= CD_MAX_PASSES &&
           guard >= 0 && guard <= CD_MAX_GUARD && floor >= 0.f && min_len >= 1 && merge_within >= 0;      // a NaN fails its comparison
}

}  // namespace

extern "C" long viai_click_detect_ws_bytes(int B, long n, int K) {
    if (!gd_shape_ok(B, n, K)) return 0;
    return (long)B * gd_tiles(n) * (long)(2 * GD_WORDS * sizeof(unsigned long long) + GD_FIELDS * sizeof(int));
}

extern "C" int viai_click_detect(const float* wav, const int* lengths, long stride, int B, long n, int order, float k, int passes, int guard,
                                 float floor, int min_len, int merge_within, int K, int* count, int* start, int* length, void* ws, void* stream) {
    if (wav == nullptr || count == nullptr || start == nullptr || length == nullptr || ws == nullptr || !gd_shape_ok(B, n, K) ||
        !cd_rule_ok(stride, n, order, k, passes, guard, floor, min_len, merge_within) || (reinterpret_cast<uintptr_t>(wav) & 3) != 0 ||
        (reinterpret_cast<uintptr_t>(ws) & 7) != 0)
        return (int)hipErrorInvalidValue;
    const long ntiles = gd_tiles(n), tiles_total = (long)B * ntiles;
    unsigned long long* flags = static_cast<unsigned long long*>(ws);
    unsigned long long* mask = flags + tiles_total * GD_WORDS;
    int* tab = reinterpret_cast<int*>(mask + tiles_total * GD_WORDS);
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = CD_LDS_DOUBLES * sizeof(double);
    static bool attr = false;
    if (!attr) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(cd_flag_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        attr = true;
    }
    VIAI_LAUNCH(cd_flag_kernel, dim3((unsigned)tiles_total), dim3(AR_THREADS), lds, st, wav, lengths, stride, (int)n, (int)ntiles, order,
                cd_square(k), cd_square(floor), passes, flags);
    VIAI_LAUNCH(cd_dilate_kernel, dim3((unsigned)((tiles_total + GD_WAVES - 1) / GD_WAVES)), dim3(GD_THREADS), 0, st, flags, lengths, (int)n,
                (int)ntiles, guard, min_len, merge_within, mask, tab, tiles_total);
    const int e = viai_launch_status();
    const int e2 = viai_gd_launch_runs(lengths, (int)n, (int)ntiles, min_len, merge_within, K, mask, tab, tiles_total, count, start, length, st);
    return e != 0 ? e : e2;
}

// The same rule with plain loops from the same headers, every pointer in HOST memory: tiles only where the fit needs them, then flags, dilation and
// runs sample by sample.
extern "C" int viai_click_detect_host(const float* wav, const int* lengths, long stride, int B, long n, int order, float k, int passes, int guard,
                                      float floor, int min_len, int merge_within, int K, int* count, int* start, int* length) {
    if (wav == nullptr || count == nullptr || start == nullptr || length == nullptr || !gd_shape_ok(B, n, K) ||
        !cd_rule_ok(stride, n, order, k, passes, guard, floor, min_len, merge_within))
        return (int)hipErrorInvalidValue;
    const double kk = cd_square(k), ff = cd_square(floor);
    std::vector<double> x(GD_TILE), F(GD_TILE), Bk(GD_TILE), q(GD_TILE);
    std::vector<char> judged(GD_TILE), flag, mask;
    for (int b = 0; b < B; ++b) {
        const float* xr = wav + (long)b * stride;
        const long len = ar_row_len(lengths, b, n);
        flag.assign((size_t)len, 0);
        mask.assign((size_t)len, 0);
        for (long t0 = 0; t0 < len; t0 += GD_TILE) {
            const long C = len - t0 < GD_TILE ? len - t0 : GD_TILE;
            const int p = cd_order(order, C);
            for (long i = 0; i < C; ++i)
                if (cd_nonfinite(xr[t0 + i])) flag[t0 + i] = 1;
            if (p < 1) continue;
            double a[AR_COEF];
            for (long i = 0; i < C; ++i) x[i] = ar_sample(xr[t0 + i]);
            ar_fit_plain(x.data(), C, p, a, F.data(), Bk.data());
            for (long i = 0; i < C; ++i) {
                judged[i] = t0 + i >= p;
                if (!judged[i]) continue;
                const double e = cd_residual(a, p, xr + t0 + i);
                q[i] = e * e;
            }
            double var = 0.0;
            for (int r = 0; r <= passes; ++r) {
                double part[CD_PARTS];
                long cnt = 0;
                for (int t = 0; t < CD_PARTS; ++t) {
                    double acc = 0.0;
                    for (long i = t; i < C; i += CD_PARTS) {
                        if (judged[i] && (r == 0 || cd_keep(q[i], kk, var))) {
                            acc = cd_add(acc, q[i]);
                            ++cnt;
                        }
                    }
                    part[t] = acc;
                }
                var = cd_mean(ar_tree(part, CD_PARTS), cnt, var);
            }
            for (long i = 0; i < C; ++i)
                if (judged[i] && cd_flag(q[i], kk, var, ff)) flag[t0 + i] = 1;
        }
        for (long j = 0; j < len; ++j) {
            if (!flag[j]) continue;
            const long lo = j - guard > 0 ? j - guard : 0, hi = j + guard < len - 1 ? j + guard : len - 1;
            for (long i = lo; i <= hi; ++i) mask[i] = 1;
        }
        count[b] = gd_runs_host(len, [&](long i) { return mask[i] != 0; }, min_len, merge_within, K, start + (long)b * K, length + (long)b * K);
    }
    return 0;
}
