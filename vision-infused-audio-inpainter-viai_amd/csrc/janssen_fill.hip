// Crackle and short gaps (gfx950): Janssen's least-squares AR interpolation of every cluster of listed runs of every row, in one launch.
// Contract and rule: include/viai_hip.h; the arithmetic, with the order of every sum: viai_janssen_rule.h (on viai_ar_rule.h); launch shape, LDS
// budget, serial depth and what is measured: DESIGN.md 11.2s.
//
// One block of 256 threads per (row, entry index).  Every thread walks the row's list (jn_plan: integers only); the block whose entry opens a
// cluster does that cluster, every other block returns before any barrier (a skipped entry's block writes its filled = 0).  The leader:
//   1  the window goes into LDS as fp64 with 0.0 at the unknowns (X0), the unknowns' positions into T, the estimates Y start at 0.0
//   2  per iteration: F = B = X0 with Y scattered in; Burg on the whole window (ar_burg_block<1>, the fit of ar_fill, unchanged)
//   3  b_l by thread l; then the band of G (overlaying F and B, which the fit is done with) and the right-hand side, an element a thread
//   4  L D L^T column by column: (b) threads q < cnt divide column j and take the forward substitution along, (c) the block applies the
//      column's outer product to the cnt (cnt + 1) / 2 elements behind it.  Two barriers a column; the pivot test reads LDS behind a
//      barrier, so the whole block leaves together
//   5  y = z / d by the block, the back substitution by wave 0 alone (lane q the rows j - 1 - q and j - 65 - q: LDS operations of one wave
//      stay in order), Y <- the solution
//   6  fp32 stores at the unknowns only, filled of every member
// No atomics, no global workspace, nothing synced with the host.  wav and out may be the same pointer: a block reads only its own window,
// which holds no unknown of another cluster, and writes only its own unknowns.
#include <vector>

#include "viai_common.h"
#include "viai_janssen_rule.h"
#include "viai_ar_fit.h"

#pragma clang fp contract(off)

namespace {

// LDS, in doubles: X0 | F B (the band overlays them) | Z | Y | COL | BC | coef[2][AR_COEF], red[4][3] | then M ints of T
constexpr int JN_OFF_FB = JN_MAX_WINDOW;
constexpr int JN_OFF_Z = JN_OFF_FB + 2 * JN_MAX_WINDOW;
constexpr int JN_OFF_Y = JN_OFF_Z + JN_MAX_UNKNOWN;
constexpr int JN_OFF_COL = JN_OFF_Y + JN_MAX_UNKNOWN;
constexpr int JN_OFF_BC = JN_OFF_COL + AR_MAX_ORDER;
constexpr int JN_OFF_COEF = JN_OFF_BC + AR_MAX_ORDER + 8;                       // b_0 .. b_128 and padding
constexpr int JN_OFF_T = JN_OFF_COEF + ar_small_doubles(1);
constexpr size_t JN_LDS_BYTES = (size_t)JN_OFF_T * sizeof(double) + (size_t)JN_MAX_UNKNOWN * sizeof(int);
static_assert(2 * JN_MAX_WINDOW >= JN_BAND_DOUBLES, "the band overlays F and B");
static_assert(JN_MAX_WINDOW <= AR_MAX_CONTEXT, "the fit's longest input");
static_assert(JN_LDS_BYTES <= 160 * 1024, "gfx950: 160 KB of LDS a workgroup");

__global__ __launch_bounds__(AR_THREADS) void janssen_fill_kernel(const float* wav, const int* __restrict__ lengths, long stride, long n,
                                                                  const int* __restrict__ count, const int* __restrict__ start,
                                                                  const int* __restrict__ length, int K, int order, int context, int max_len,
                                                                  int iters, float* out, long out_stride, int* __restrict__ filled) {
    extern __shared__ double lds[];
    const int b = blockIdx.x / K, k = blockIdx.x - b * K;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int cnt_b = count[b], listed = cnt_b < K ? (cnt_b < 0 ? 0 : cnt_b) : K;
    const int* st = start + (long)b * K;
    const int* ln = length + (long)b * K;
    const JnPlan pl = jn_plan(st, ln, k, listed, ar_row_len(lengths, b, n), order, context, max_len);
    if (pl.leader != k) {                                                      // the whole block: no barrier has been reached
        if (pl.leader < 0 && tid == 0) filled[(long)b * K + k] = AR_SKIPPED;
        return;
    }
    const float* xr = wav + (long)b * stride + pl.lo;
    const int W = (int)(pl.hi - pl.lo), M = (int)pl.M;
    const int p = W / 2 < order ? W / 2 : order;
    double* X0 = lds;
    double* FB = lds + JN_OFF_FB;
    double* Z = lds + JN_OFF_Z;
    double* Y = lds + JN_OFF_Y;
    double* COL = lds + JN_OFF_COL;
    double* BC = lds + JN_OFF_BC;
    double* coef = lds + JN_OFF_COEF;
    double* red = coef + 2 * AR_COEF;
    int* T = reinterpret_cast<int*>(lds + JN_OFF_T);

    // 1  the window, the unknowns' positions, zeros
    for (int j = tid; j < W; j += AR_THREADS) X0[j] = ar_sample(xr[j]);
    {
        int off = 0;
        for (int m = k; m <= pl.last; ++m) {
            const int s = (int)((long)st[m] - pl.lo), L = ln[m];
            for (int q = tid; q < L; q += AR_THREADS) T[off + q] = s + q;
            off += L;
        }
    }
    __syncthreads();
    for (int i = tid; i < M; i += AR_THREADS) {
        X0[T[i]] = 0.0;
        Y[i] = 0.0;
    }
    __syncthreads();

    int code = JN_SOLVED;
    if (p < 1) code = AR_NONE;
    const int pw = p + 1;                                                      // doubles a band row
    for (int it = 0; it < iters && code == JN_SOLVED; ++it) {
        // 2  the fit on the window with the current estimates
        for (int j = tid; j < W; j += AR_THREADS) {
            const double x = X0[j];
            FB[j] = x;
            FB[JN_MAX_WINDOW + j] = x;
        }
        if (tid == 0) coef[0] = 1.0;
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

        // 3  b_l, then the band and the right-hand side
        if (tid <= p) BC[tid] = jn_autocorr(a, p, tid);
        __syncthreads();
        double* band = FB;
        for (int idx = tid; idx < M * pw; idx += AR_THREADS) {
            const int i = idx / pw, c = idx - i * pw, j = i - p + c;
            band[idx] = j < 0 ? 0.0 : jn_gram(BC, p, (long)(T[i] - T[j]));
        }
        for (int i = tid; i < M; i += AR_THREADS) Z[i] = jn_rhs(BC, p, X0, W, T[i]);
        __syncthreads();

        // 4  L D L^T with the forward substitution
        for (int j = 0; j < M; ++j) {
            const double d = band[jn_at(j, j, p)];                             // the same LDS word for every thread, behind a barrier
            if (!jn_pivot_ok(d)) {
                code = JN_PIVOT;
                break;
            }
            const int cnt = M - 1 - j < p ? M - 1 - j : p;
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
        if (code != JN_SOLVED) break;                                          // Y keeps the last completed iteration

        // 5  divide, back substitution by wave 0, the new estimates
        for (int i = tid; i < M; i += AR_THREADS) Z[i] = jn_div(Z[i], band[jn_at(i, i, p)]);
        __syncthreads();
        if (wv == 0) {
            for (int j = M - 1; j >= 1; --j) {
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
        for (int i = tid; i < M; i += AR_THREADS) Y[i] = Z[i];
        __syncthreads();
    }

    // 6  fp32 stores at the unknowns only
    float* yr = out + (long)b * out_stride + pl.lo;
    for (int i = tid; i < M; i += AR_THREADS) yr[T[i]] = (float)Y[i];
    for (int m = k + tid; m <= pl.last; m += AR_THREADS) filled[(long)b * K + m] = code;
}

inline bool jn_limits_ok(int order, int context, int max_len, int iters) {
    return order >= 1 && order <= AR_MAX_ORDER && context >= 2 && context <= JN_MAX_CONTEXT && iters >= 1 && iters <= JN_MAX_ITERS &&
           max_len >= 1 && max_len <= jn_max_len(order, context);
}

inline bool jn_lists_ok(int B, long n, const int* count, const int* start, const int* length, int K) {
    return count != nullptr && start != nullptr && length != nullptr && B >= 1 && K >= 1 && n >= 1 && n < (1L << 31) &&
           (long)B * K <= 0x7fffffffL;
}

inline bool jn_args_ok(const float* wav, long stride, int B, long n, const int* count, const int* start, const int* length, int K, int order,
                       int context, int max_len, int iters, const float* out, long out_stride, const int* filled) {
    return wav != nullptr && out != nullptr && filled != nullptr && jn_lists_ok(B, n, count, start, length, K) && stride >= n &&
           out_stride >= n && jn_limits_ok(order, context, max_len, iters);
}

inline int jn_listed(const int* count, int b, int K) {
    const int c = count[b];
    return c < K ? (c < 0 ? 0 : c) : K;
}

}  // namespace

extern "C" int viai_janssen_fill(const float* wav, const int* lengths, long stride, int B, long n, const int* count, const int* start,
                                 const int* length, int K, int order, int context, int max_len, int iters, float* out, long out_stride,
                                 int* filled, void* stream) {
    if (!jn_args_ok(wav, stride, B, n, count, start, length, K, order, context, max_len, iters, out, out_stride, filled) ||
        (reinterpret_cast<uintptr_t>(wav) & 3) != 0 || (reinterpret_cast<uintptr_t>(out) & 3) != 0)
        return (int)hipErrorInvalidValue;
    static bool attr = false;
    if (!attr) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(janssen_fill_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)JN_LDS_BYTES);
        attr = true;
    }
    VIAI_LAUNCH(janssen_fill_kernel, dim3((unsigned)((long)B * K)), dim3(AR_THREADS), JN_LDS_BYTES, (hipStream_t)stream, wav, lengths, stride,
                n, count, start, length, K, order, context, max_len, iters, out, out_stride, filled);
    return viai_launch_status();
}

// The same rule with plain loops, every pointer in HOST memory.
extern "C" int viai_janssen_fill_host(const float* wav, const int* lengths, long stride, int B, long n, const int* count, const int* start,
                                      const int* length, int K, int order, int context, int max_len, int iters, float* out, long out_stride,
                                      int* filled) {
    if (!jn_args_ok(wav, stride, B, n, count, start, length, K, order, context, max_len, iters, out, out_stride, filled))
        return (int)hipErrorInvalidValue;
    std::vector<double> x0(JN_MAX_WINDOW), x(JN_MAX_WINDOW), F(JN_MAX_WINDOW), Bk(JN_MAX_WINDOW), band(JN_BAND_DOUBLES), z(JN_MAX_UNKNOWN),
        y(JN_MAX_UNKNOWN), col(AR_MAX_ORDER), bc(AR_COEF);
    std::vector<int> t(JN_MAX_UNKNOWN);
    for (int b = 0; b < B; ++b) {
        const int* st = start + (long)b * K;
        const int* ln = length + (long)b * K;
        const int listed = jn_listed(count, b, K);
        const long len = ar_row_len(lengths, b, n);
        for (int k = 0; k < K; ++k) {
            const JnPlan pl = jn_plan(st, ln, k, listed, len, order, context, max_len);
            if (pl.leader < 0) filled[(long)b * K + k] = AR_SKIPPED;
            if (pl.leader != k) continue;
            const float* xr = wav + (long)b * stride + pl.lo;
            const long W = pl.hi - pl.lo, M = pl.M;
            const int p = (int)(W / 2 < order ? W / 2 : order);
            for (long j = 0; j < W; ++j) x0[j] = ar_sample(xr[j]);
            long off = 0;
            for (int m = k; m <= pl.last; ++m)
                for (int q = 0; q < ln[m]; ++q) t[off++] = (int)((long)st[m] - pl.lo) + q;
            for (long i = 0; i < M; ++i) {
                x0[t[i]] = 0.0;
                y[i] = 0.0;
            }
            int code = p < 1 ? AR_NONE : JN_SOLVED;
            for (int it = 0; it < iters && code == JN_SOLVED; ++it) {
                double a[AR_COEF];
                for (long j = 0; j < W; ++j) x[j] = x0[j];
                for (long i = 0; i < M; ++i) x[t[i]] = y[i];
                ar_fit_plain(x.data(), W, p, a, F.data(), Bk.data());
                for (int l = 0; l <= p; ++l) bc[l] = jn_autocorr(a, p, l);
                jn_band_fill(band.data(), t.data(), M, p, bc.data());
                for (long i = 0; i < M; ++i) z[i] = jn_rhs(bc.data(), p, x0.data(), W, t[i]);
                if (!jn_ldl_plain(band.data(), M, p, z.data(), col.data())) {
                    code = JN_PIVOT;
                    break;
                }
                for (long i = 0; i < M; ++i) y[i] = z[i];
            }
            float* yr = out + (long)b * out_stride + pl.lo;
            for (long i = 0; i < M; ++i) yr[t[i]] = (float)y[i];
            for (int m = k; m <= pl.last; ++m) filled[(long)b * K + m] = code;
        }
    }
    return 0;
}

// The cluster rule alone, every pointer in HOST memory: per entry the leader's index (-1: skipped), the window [lo, hi) and M.
extern "C" int viai_janssen_plan_host(const int* lengths, int B, long n, const int* count, const int* start, const int* length, int K, int order,
                                      int context, int max_len, int* leader, int* win_lo, int* win_hi, int* unknowns) {
    if (leader == nullptr || win_lo == nullptr || win_hi == nullptr || unknowns == nullptr || !jn_lists_ok(B, n, count, start, length, K) ||
        !jn_limits_ok(order, context, max_len, 1))
        return (int)hipErrorInvalidValue;
    for (int b = 0; b < B; ++b)
        for (int k = 0; k < K; ++k) {
            const JnPlan pl = jn_plan(start + (long)b * K, length + (long)b * K, k, jn_listed(count, b, K), ar_row_len(lengths, b, n), order,
                                      context, max_len);
            const long o = (long)b * K + k;
            leader[o] = pl.leader;
            win_lo[o] = (int)pl.lo;
            win_hi[o] = (int)pl.hi;
            unknowns[o] = (int)pl.M;
        }
    return 0;
}
