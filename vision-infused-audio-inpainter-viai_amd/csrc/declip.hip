// Declipping (gfx950): bound-constrained Janssen AR restoration of every cluster of listed runs of every row, one launch per sweep.
// Contract and rule: include/viai_hip.h; the arithmetic, with the order of every sum: viai_declip_rule.h (on viai_janssen_rule.h and
// viai_ar_rule.h); launch shape, LDS budget, serial depth and what is measured: DESIGN.md 11.2t.
//
// One block of 256 threads per (row, entry index), the shape of janssen_fill_kernel: every thread walks the row's list (dc_plan: integers
// only); the block whose entry opens a cluster does that cluster, every other block returns before any barrier.  The leader:
//   1  the window of `src` goes into LDS as fp64 (X0), the unknowns' positions into T, the bounds C from `ref`; the estimates Y start at
//      src's samples, then X0 gets 0.0 at the unknowns
//   2  per iteration: Burg on the window with Y in place (ar_burg_block<1>, unchanged), b_l by thread l
//   3  dc_solve_block over all M unknowns: the band (overlaying F and B) and the right-hand side an element a thread, L D L^T column by
//      column with two barriers a column, the back substitution by wave 0: the loops of janssen_fill_kernel, copied
//   4  up to `rounds` times: every free unknown that violates its bound is pinned (its wave ORs a ballot into the wave's own word of the pin
//      bitmap, X0 gets c there), the free ones are compacted into TF by ballots and a four-wave exclusive sum, and dc_solve_block runs again
//      over TF.  "Any pinned?" and the free count are read from LDS behind a barrier: the whole block takes the same branch
//   5  clamp, Y <- the estimates, X0 back to 0.0 at the unknowns
//   6  fp32 stores at the unknowns only, filled of every member
// No atomics, no global workspace, nothing synced with the host.  out must not overlap src or ref: a window holds samples of OTHER clusters'
// entries, which their blocks write in this same launch.
#include <vector>

#include "viai_common.h"
#include "viai_declip_rule.h"
#include "viai_ar_fit.h"

#pragma clang fp contract(off)

namespace {

// LDS, in doubles: X0 | F B (the band overlays them) | Z | Y | X | C | COL | BC | coef[2][AR_COEF], red[4][3] | PIN (16 words) | then the ints
// T[1024], TF[1024], WC[4], WN[4]
constexpr int DC_OFF_FB = JN_MAX_WINDOW;
constexpr int DC_OFF_Z = DC_OFF_FB + 2 * JN_MAX_WINDOW;
constexpr int DC_OFF_Y = DC_OFF_Z + JN_MAX_UNKNOWN;
constexpr int DC_OFF_X = DC_OFF_Y + JN_MAX_UNKNOWN;
constexpr int DC_OFF_C = DC_OFF_X + JN_MAX_UNKNOWN;
constexpr int DC_OFF_COL = DC_OFF_C + JN_MAX_UNKNOWN;
constexpr int DC_OFF_BC = DC_OFF_COL + AR_MAX_ORDER;
constexpr int DC_OFF_COEF = DC_OFF_BC + AR_MAX_ORDER + 8;                       // b_0 .. b_128 and padding
constexpr int DC_OFF_PIN = DC_OFF_COEF + ar_small_doubles(1);
constexpr int DC_PIN_WORDS = JN_MAX_UNKNOWN / 64;
constexpr int DC_OFF_T = DC_OFF_PIN + DC_PIN_WORDS;
constexpr size_t DC_LDS_BYTES = (size_t)DC_OFF_T * sizeof(double) + (size_t)(2 * JN_MAX_UNKNOWN + 8) * sizeof(int);
static_assert(2 * JN_MAX_WINDOW >= JN_BAND_DOUBLES, "the band overlays F and B");
static_assert(JN_MAX_WINDOW <= AR_MAX_CONTEXT, "the fit's longest input");
static_assert(JN_MAX_UNKNOWN % AR_THREADS == 0 && AR_THREADS == 4 * 64, "a wave's 64 unknowns of a pass are one word of the pin bitmap");
static_assert(DC_LDS_BYTES <= 160 * 1024, "gfx950: 160 KB of LDS a workgroup");

// Band, right-hand side, L D L^T with the forward substitution, divide, back substitution over the Mx unknowns at positions T[TF[i]] (TF ==
// nullptr: T[i]); the solution is left in Z[0 .. Mx).  Every thread of the block calls it behind a barrier; it ends behind one.  false: a
// pivot was not > 0.0 or not finite (read from LDS behind a barrier: the whole block returns together).
__device__ __forceinline__ bool dc_solve_block(double* band, double* Z, double* COL, const double* BC, const double* X0, const int* T,
                                               const int* TF, int Mx, int p, int W) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int pw = p + 1;                                                      // doubles a band row
    for (int idx = tid; idx < Mx * pw; idx += AR_THREADS) {
        const int i = idx / pw, c = idx - i * pw, j = i - p + c;
        band[idx] = j < 0 ? 0.0 : jn_gram(BC, p, (long)(dc_pos(T, TF, i) - dc_pos(T, TF, j)));
    }
    for (int i = tid; i < Mx; i += AR_THREADS) Z[i] = jn_rhs(BC, p, X0, W, dc_pos(T, TF, i));
    __syncthreads();
    for (int j = 0; j < Mx; ++j) {
        const double d = band[jn_at(j, j, p)];                                 // the same LDS word for every thread, behind a barrier
        if (!jn_pivot_ok(d)) return false;
        const int cnt = Mx - 1 - j < p ? Mx - 1 - j : p;
        if (tid < cnt) {
            const int i = j + 1 + tid;
            const double c = band[jn_at(i, j, p)], l = jn_div(c, d);
            COL[tid] = c;
            band[jn_at(i, j, p)] = l;
            Z[i] = jn_down(Z[i], l, Z[j]);
        }
        __syncthreads();
        for (int idx = tid; idx < cnt * cnt; idx += AR_THREADS) {
            const int qi = idx / cnt, qk = idx - qi * cnt;
            if (qk <= qi) {
                const int i = j + 1 + qi, kk = j + 1 + qk;
                band[jn_at(i, kk, p)] = jn_down(band[jn_at(i, kk, p)], band[jn_at(i, j, p)], COL[qk]);
            }
        }
        __syncthreads();
    }
    for (int i = tid; i < Mx; i += AR_THREADS) Z[i] = jn_div(Z[i], band[jn_at(i, i, p)]);
    __syncthreads();
    if (wv == 0) {
        for (int j = Mx - 1; j >= 1; --j) {
            const double xj = Z[j];
            const int cnt = j < p ? j : p;
            if (lane < cnt) Z[j - 1 - lane] = jn_down(Z[j - 1 - lane], band[jn_at(j, j - 1 - lane, p)], xj);
            if (lane + AR_LANES < cnt) Z[j - 65 - lane] = jn_down(Z[j - 65 - lane], band[jn_at(j, j - 65 - lane, p)], xj);
            // the next step's lanes read what other lanes wrote: same wave, LDS operations in order; keep the compiler from moving them
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
    }
    __syncthreads();
    return true;
}

__global__ __launch_bounds__(AR_THREADS) void declip_kernel(const float* ref, const float* src, const int* __restrict__ lengths, long stride,
                                                            long n, const int* __restrict__ count, const int* __restrict__ start,
                                                            const int* __restrict__ length, int K, int order, int context, int max_len,
                                                            int iters, int rounds, float* out, long out_stride, int* __restrict__ filled) {
    extern __shared__ double lds[];
    const int b = blockIdx.x / K, k = blockIdx.x - b * K;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int cnt_b = count[b], listed = cnt_b < K ? (cnt_b < 0 ? 0 : cnt_b) : K;
    const int* st = start + (long)b * K;
    const int* ln = length + (long)b * K;
    const JnPlan pl = dc_plan(st, ln, k, listed, ar_row_len(lengths, b, n), order, context, max_len);
    if (pl.leader != k) {                                                      // the whole block: no barrier has been reached
        if (pl.leader < 0 && tid == 0) filled[(long)b * K + k] = AR_SKIPPED;
        return;
    }
    const float* xs = src + (long)b * stride + pl.lo;
    const float* xr = ref + (long)b * stride + pl.lo;
    const int W = (int)(pl.hi - pl.lo), M = (int)pl.M;
    const int p = W / 2 < order ? W / 2 : order;
    double* X0 = lds;
    double* FB = lds + DC_OFF_FB;
    double* Z = lds + DC_OFF_Z;
    double* Y = lds + DC_OFF_Y;
    double* X = lds + DC_OFF_X;
    double* Cb = lds + DC_OFF_C;
    double* COL = lds + DC_OFF_COL;
    double* BC = lds + DC_OFF_BC;
    double* coef = lds + DC_OFF_COEF;
    double* red = coef + 2 * AR_COEF;
    unsigned long long* PIN = reinterpret_cast<unsigned long long*>(lds + DC_OFF_PIN);
    int* T = reinterpret_cast<int*>(lds + DC_OFF_T);
    int* TF = T + JN_MAX_UNKNOWN;
    int* WC = TF + JN_MAX_UNKNOWN;
    int* WN = WC + 4;

    // 1  the window, the unknowns' positions, their bounds and start values
    for (int j = tid; j < W; j += AR_THREADS) X0[j] = ar_sample(xs[j]);
    {
        int off = 0;
        for (int m = k; m <= pl.last; ++m) {
            const int s = (int)((long)st[m] - pl.lo), L = ln[m];
            for (int q = tid; q < L; q += AR_THREADS) T[off + q] = s + q;
            off += L;
        }
    }
    __syncthreads();
    for (int i = tid; i < M; i += AR_THREADS) {                                // the positions are distinct: thread i alone touches X0[T[i]]
        const int t = T[i];
        Cb[i] = ar_sample(xr[t]);
        Y[i] = X0[t];
        X0[t] = 0.0;
    }
    __syncthreads();

    int code = JN_SOLVED;
    if (p < 1) code = AR_NONE;
    for (int it = 0; it < iters && code == JN_SOLVED; ++it) {
        // 2  the fit on the window with the current estimates, then b_l
        for (int j = tid; j < W; j += AR_THREADS) {
            const double x = X0[j];
            FB[j] = x;
            FB[JN_MAX_WINDOW + j] = x;
        }
        if (tid == 0) coef[0] = 1.0;
        if (tid < DC_PIN_WORDS) PIN[tid] = 0ull;                               // pins are cleared at every fit
        __syncthreads();
        for (int i = tid; i < M; i += AR_THREADS) {
            const double y = Y[i];
            FB[T[i]] = y;
            FB[JN_MAX_WINDOW + T[i]] = y;
        }
        __syncthreads();
        const long C[1] = {W};
        const int ps[1] = {p};
        int cur[1] = {0};
        ar_burg_block<1>(FB, 0L, (long)JN_MAX_WINDOW, C, ps, coef, red, cur);  // ends behind a barrier
        const double* a = coef + cur[0] * AR_COEF;
        if (tid <= p) BC[tid] = jn_autocorr(a, p, tid);
        __syncthreads();

        // 3  all M unknowns
        if (!dc_solve_block(FB, Z, COL, BC, X0, T, nullptr, M, p, W)) {
            code = JN_PIVOT;
            break;                                                             // Y keeps the last completed iteration
        }
        for (int i = tid; i < M; i += AR_THREADS) X[i] = Z[i];
        __syncthreads();

        // 4  pin, compact, solve the free ones again
        for (int r = 0; r < rounds; ++r) {
            int run = 0;
            bool anyw = false;
            for (int base = 0; base < M; base += AR_THREADS) {
                const int i = base + tid, word = i >> 6;                       // i & 63 == lane: the wave's 64 unknowns are one word
                const unsigned long long old = PIN[word];
                const bool open = i < M && ((old >> lane) & 1ull) == 0;
                bool nw = false;
                if (open) {
                    const double c = Cb[i];
                    nw = dc_violates(c, X[i]);
                    if (nw) {
                        X[i] = c;
                        X0[T[i]] = c;                                          // a known of value c in the next right-hand side
                    }
                }
                const unsigned long long bn = __ballot(nw);
                const bool fr = open && !nw;
                const unsigned long long bf = __ballot(fr);
                anyw = anyw || bn != 0ull;
                if (lane == 0) {
                    PIN[word] = old | bn;
                    WC[wv] = __popcll(bf);
                }
                __syncthreads();
                const int c0 = WC[0], c1 = WC[1], c2 = WC[2], c3 = WC[3];
                const int before = wv == 0 ? 0 : (wv == 1 ? c0 : (wv == 2 ? c0 + c1 : c0 + c1 + c2));
                if (fr) TF[run + before + __popcll(bf & ((1ull << lane) - 1ull))] = i;
                run += c0 + c1 + c2 + c3;
                __syncthreads();
            }
            if (lane == 0) WN[wv] = anyw ? 1 : 0;
            __syncthreads();
            const bool any = (WN[0] | WN[1] | WN[2] | WN[3]) != 0;
            if (!any || run == 0) break;                                       // nothing new, or nothing left to solve for
            if (!dc_solve_block(FB, Z, COL, BC, X0, T, TF, run, p, W)) {
                code = JN_PIVOT;
                break;
            }
            for (int q = tid; q < run; q += AR_THREADS) X[TF[q]] = Z[q];
            __syncthreads();
        }
        if (code != JN_SOLVED) break;

        // 5  clamp what still violates, the new estimates, X0 back to 0.0 at the unknowns
        for (int i = tid; i < M; i += AR_THREADS) {
            const double c = Cb[i];
            double x = X[i];
            if (rounds > 0 && dc_violates(c, x)) x = c;
            Y[i] = x;
            X0[T[i]] = 0.0;
        }
        __syncthreads();
    }

    // 6  fp32 stores at the unknowns only
    float* yr = out + (long)b * out_stride + pl.lo;
    for (int i = tid; i < M; i += AR_THREADS) yr[T[i]] = (float)Y[i];
    for (int m = k + tid; m <= pl.last; m += AR_THREADS) filled[(long)b * K + m] = code;
}

inline bool dc_limits_ok(int order, int context, int max_len, int iters, int rounds) {
    return order >= 1 && order <= AR_MAX_ORDER && context >= 2 && context <= JN_MAX_CONTEXT && iters >= 1 && iters <= JN_MAX_ITERS &&
           rounds >= 0 && rounds <= DC_MAX_ROUNDS && max_len >= 1 && max_len <= jn_max_len(order, context);
}

// [a, a + (B - 1) a_stride + n) against [o, o + (B - 1) o_stride + n), in bytes
inline bool dc_overlap(const float* a, long a_stride, const float* o, long o_stride, int B, long n) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), o0 = reinterpret_cast<uintptr_t>(o);
    const uintptr_t a1 = a0 + (uintptr_t)(((long)(B - 1) * a_stride + n) * (long)sizeof(float));
    const uintptr_t o1 = o0 + (uintptr_t)(((long)(B - 1) * o_stride + n) * (long)sizeof(float));
    return a0 < o1 && o0 < a1;
}

inline bool dc_args_ok(const float* ref, const float* src, long stride, int B, long n, const int* count, const int* start, const int* length,
                       int K, int order, int context, int max_len, int iters, int rounds, const float* out, long out_stride,
                       const int* filled) {
    return ref != nullptr && src != nullptr && out != nullptr && filled != nullptr && count != nullptr && start != nullptr &&
           length != nullptr && B >= 1 && K >= 1 && n >= 1 && n < (1L << 31) && (long)B * K <= 0x7fffffffL && stride >= n && out_stride >= n &&
           dc_limits_ok(order, context, max_len, iters, rounds) && !dc_overlap(src, stride, out, out_stride, B, n) &&
           !dc_overlap(ref, stride, out, out_stride, B, n);
}

}  // namespace

extern "C" int viai_declip(const float* ref, const float* src, const int* lengths, long stride, int B, long n, const int* count, const int* start,
                           const int* length, int K, int order, int context, int max_len, int iters, int rounds, float* out, long out_stride,
                           int* filled, void* stream) {
    if (!dc_args_ok(ref, src, stride, B, n, count, start, length, K, order, context, max_len, iters, rounds, out, out_stride, filled) ||
        (reinterpret_cast<uintptr_t>(ref) & 3) != 0 || (reinterpret_cast<uintptr_t>(src) & 3) != 0 || (reinterpret_cast<uintptr_t>(out) & 3) != 0)
        return (int)hipErrorInvalidValue;
    static bool attr = false;
    if (!attr) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(declip_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)DC_LDS_BYTES);
        attr = true;
    }
    VIAI_LAUNCH(declip_kernel, dim3((unsigned)((long)B * K)), dim3(AR_THREADS), DC_LDS_BYTES, (hipStream_t)stream, ref, src, lengths, stride, n,
                count, start, length, K, order, context, max_len, iters, rounds, out, out_stride, filled);
    return viai_launch_status();
}

// The same rule with plain loops, every pointer in HOST memory.
extern "C" int viai_declip_host(const float* ref, const float* src, const int* lengths, long stride, int B, long n, const int* count,
                                const int* start, const int* length, int K, int order, int context, int max_len, int iters, int rounds,
                                float* out, long out_stride, int* filled) {
    if (!dc_args_ok(ref, src, stride, B, n, count, start, length, K, order, context, max_len, iters, rounds, out, out_stride, filled))
        return (int)hipErrorInvalidValue;
    std::vector<double> x0(JN_MAX_WINDOW), xw(JN_MAX_WINDOW), F(JN_MAX_WINDOW), Bk(JN_MAX_WINDOW), band(JN_BAND_DOUBLES), z(JN_MAX_UNKNOWN),
        y(JN_MAX_UNKNOWN), x(JN_MAX_UNKNOWN), cb(JN_MAX_UNKNOWN), col(AR_MAX_ORDER), bc(AR_COEF);
    std::vector<int> t(JN_MAX_UNKNOWN), tf(JN_MAX_UNKNOWN);
    unsigned long long pin[JN_MAX_UNKNOWN / 64];
    for (int b = 0; b < B; ++b) {
        const int* st = start + (long)b * K;
        const int* ln = length + (long)b * K;
        const int c = count[b], listed = c < K ? (c < 0 ? 0 : c) : K;
        const long len = ar_row_len(lengths, b, n);
        for (int k = 0; k < K; ++k) {
            const JnPlan pl = dc_plan(st, ln, k, listed, len, order, context, max_len);
            if (pl.leader < 0) filled[(long)b * K + k] = AR_SKIPPED;
            if (pl.leader != k) continue;
            const float* xs = src + (long)b * stride + pl.lo;
            const float* xr = ref + (long)b * stride + pl.lo;
            const long W = pl.hi - pl.lo, M = pl.M;
            const int p = (int)(W / 2 < order ? W / 2 : order);
            for (long j = 0; j < W; ++j) x0[j] = ar_sample(xs[j]);
            long off = 0;
            for (int m = k; m <= pl.last; ++m)
                for (int q = 0; q < ln[m]; ++q) t[off++] = (int)((long)st[m] - pl.lo) + q;
            for (long i = 0; i < M; ++i) {
                cb[i] = ar_sample(xr[t[i]]);
                y[i] = x0[t[i]];
                x0[t[i]] = 0.0;
            }
            int code = p < 1 ? AR_NONE : JN_SOLVED;
            for (int it = 0; it < iters && code == JN_SOLVED; ++it) {
                double a[AR_COEF];
                for (long j = 0; j < W; ++j) xw[j] = x0[j];
                for (long i = 0; i < M; ++i) xw[t[i]] = y[i];
                for (int w = 0; w < JN_MAX_UNKNOWN / 64; ++w) pin[w] = 0ull;
                ar_fit_plain(xw.data(), W, p, a, F.data(), Bk.data());
                for (int l = 0; l <= p; ++l) bc[l] = jn_autocorr(a, p, l);
                dc_band_fill(band.data(), t.data(), nullptr, M, p, bc.data());
                for (long i = 0; i < M; ++i) z[i] = jn_rhs(bc.data(), p, x0.data(), W, t[i]);
                if (!jn_ldl_plain(band.data(), M, p, z.data(), col.data())) {
                    code = JN_PIVOT;
                    break;
                }
                for (long i = 0; i < M; ++i) x[i] = z[i];
                for (int r = 0; r < rounds; ++r) {
                    bool any = false;
                    long Mf = 0;
                    for (long i = 0; i < M; ++i) {
                        if (dc_pinned(pin, (int)i)) continue;
                        if (dc_violates(cb[i], x[i])) {
                            pin[i >> 6] |= 1ull << (i & 63);
                            x[i] = cb[i];
                            x0[t[i]] = cb[i];
                            any = true;
                        } else {
                            tf[Mf++] = (int)i;
                        }
                    }
                    if (!any || Mf == 0) break;
                    dc_band_fill(band.data(), t.data(), tf.data(), Mf, p, bc.data());
                    for (long q = 0; q < Mf; ++q) z[q] = jn_rhs(bc.data(), p, x0.data(), W, t[tf[q]]);
                    if (!jn_ldl_plain(band.data(), Mf, p, z.data(), col.data())) {
                        code = JN_PIVOT;
                        break;
                    }
                    for (long q = 0; q < Mf; ++q) x[tf[q]] = z[q];
                }
                if (code != JN_SOLVED) break;
                for (long i = 0; i < M; ++i) {
                    double v = x[i];
                    if (rounds > 0 && dc_violates(cb[i], v)) v = cb[i];
                    y[i] = v;
                    x0[t[i]] = 0.0;
                }
            }
            float* yr = out + (long)b * out_stride + pl.lo;
            for (long i = 0; i < M; ++i) yr[t[i]] = (float)y[i];
            for (int m = k; m <= pl.last; ++m) filled[(long)b * K + m] = code;
        }
    }
    return 0;
}
