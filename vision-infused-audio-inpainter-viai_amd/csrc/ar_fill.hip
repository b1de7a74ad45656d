// Short gaps (gfx950): Burg autoregressive interpolation of every listed gap of every row of a batch, in one launch.
// Contract and rule: include/viai_hip.h; the arithmetic, with the order of every sum: viai_ar_rule.h; launch shape, LDS budget, serial depth and
// what is measured: DESIGN.md 11.2q.
//
// One block of 256 threads per (row, gap index); a block whose gap is not listed or is skipped writes filled = 0 and returns.  Otherwise:
//   1  both contexts go into LDS as fp64, the right one time-reversed: F = B = x per side
//   2  the two Burg recursions run TOGETHER, stage by stage: thread t owns the pairs (F[i + m + 1], B[i]), i = t, t + 256, ... of stage m, so
//      its partial of each dot product is partial t of the rule and the elementwise update touches nothing another thread owns in that pass;
//      the tree is four DPP stages and four readlanes per wave (wave_sum_d_dpp: the adjacent pairwise tree of the rule) and
//      (w0 + w1) + (w2 + w3) over the waves.  Two barriers per stage.
//   3  the predictions overlay the fit's arrays: wave 0 extrapolates forward from the left, wave 1 backward from the right at the same time,
//      L serial steps each, a step being one wave-wide p-term product (lane l the terms l + 1 and l + 65) and the same tree
//   4  the block blends and stores fp32 at the gap's samples only
// No atomics, no global workspace, nothing synced with the host.  wav and out may be the same pointer: a block reads only its two contexts,
// which hold no sample of a listed gap, and blocks write only samples of listed gaps.
#include <cmath>
#include <vector>

#include "viai_common.h"
#include "viai_ar_rule.h"
#include "viai_ar_fit.h"                                         // the stage loop of the fit and its plain-loop form: shared with click_detect.hip

#pragma clang fp contract(off)

namespace {

constexpr int AR_SMALL = ar_small_doubles(2);                   // doubles behind the big region: a[side][buffer][AR_COEF], red[wave][6]

inline long ar_big_doubles(int context, int max_len) {
    const long fit = 4L * context, pred = 2L * (AR_MAX_ORDER + max_len);
    return fit > pred ? fit : pred;
}
inline size_t ar_lds_bytes(int context, int max_len) { return (size_t)(ar_big_doubles(context, max_len) + AR_SMALL) * sizeof(double); }

__global__ __launch_bounds__(AR_THREADS) void ar_fill_kernel(const float* wav, const int* __restrict__ lengths, long stride, long n,
                                                             const int* __restrict__ count, const int* __restrict__ start,
                                                             const int* __restrict__ length, int K, int order, int context, int max_len,
                                                             long big, float* out, long out_stride, int* __restrict__ filled) {
    extern __shared__ double lds[];
    const int b = blockIdx.x / K, k = blockIdx.x - b * K;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int cnt = count[b], listed = cnt < K ? (cnt < 0 ? 0 : cnt) : K;
    const ArGap g = ar_gap(start + (long)b * K, length + (long)b * K, k, listed, ar_row_len(lengths, b, n), order, context, max_len);
    if (g.code == AR_SKIPPED) {                                                // the whole block: no barrier has been reached
        if (tid == 0) filled[(long)b * K + k] = AR_SKIPPED;
        return;
    }
    const float* xr = wav + (long)b * stride;
    const long e = g.s + g.L;
    const long C[2] = {g.cl, g.cr};
    const int p[2] = {g.pl, g.pr};
    double* coef = lds + big;                                                  // [side][buffer][AR_COEF]
    double* red = coef + 2 * 2 * AR_COEF;                                      // [wave][6]
    int cur[2] = {0, 0};

    // 1  the contexts; an unusable side is not staged
    for (int s = 0; s < 2; ++s) {
        if (p[s] < 1) continue;
        double* F = lds + (long)s * 2 * context;
        double* B = F + context;
        for (long j = tid; j < C[s]; j += AR_THREADS) {
            const double x = ar_sample(s == 0 ? xr[g.lo + j] : xr[e + C[1] - 1 - j]);
            F[j] = x;
            B[j] = x;
        }
        if (tid == 0) coef[(s * 2) * AR_COEF] = 1.0;
    }
    __syncthreads();

    // 2  the two fits (viai_ar_fit.h)
    ar_burg_block<2>(lds, 2L * context, (long)context, C, p, coef, red, cur);

    // 3  seeds (the last p context samples, read again: the fit has overwritten its arrays), then the two extrapolations
    double* P0 = lds + AR_MAX_ORDER;                                           // P[-j], j <= p: the context; P[i], i < L: the prediction
    double* P1 = P0 + AR_MAX_ORDER + max_len;
    if (tid < p[0]) P0[-(tid + 1)] = ar_sample(xr[g.s - (tid + 1)]);
    if (tid >= AR_MAX_ORDER && tid - AR_MAX_ORDER < p[1]) P1[-(tid - AR_MAX_ORDER + 1)] = ar_sample(xr[e + (tid - AR_MAX_ORDER)]);
    __syncthreads();
    if (wv < 2 && p[wv] >= 1) {
        const int ps = p[wv];
        const double* a = coef + (wv * 2 + cur[wv]) * AR_COEF;
        double* P = wv == 0 ? P0 : P1;
        const int j1 = lane + 1, j2 = lane + 1 + AR_LANES;
        const bool h1 = j1 <= ps, h2 = j2 <= ps;
        const double a1 = h1 ? a[j1] : 0.0, a2 = h2 ? a[j2] : 0.0;
        for (long i = 0; i < g.L; ++i) {
            const double t = ar_term2(h1, a1, h1 ? P[i - j1] : 0.0, h2, a2, h2 ? P[i - j2] : 0.0);
            const double sum = wave_sum_d_dpp(t);                             // the whole wave is here
            if (lane == 0) P[i] = ar_step_value(sum);
            // the next step's lanes read what lane 0 wrote: same wave, LDS operations in order; keep the compiler from moving them
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
    }
    __syncthreads();

    // 4  blend, fp32 stores at the gap's samples only
    float* yr = out + (long)b * out_stride + g.s;
    for (long i = tid; i < g.L; i += AR_THREADS) {
        const double fwd = p[0] >= 1 ? P0[i] : 0.0, bwd = p[1] >= 1 ? P1[g.L - 1 - i] : 0.0;
        yr[i] = ar_blend(g.code, i, g.L, fwd, bwd);
    }
    if (tid == 0) filled[(long)b * K + k] = g.code;
}

inline bool ar_limits_ok(int order, int context, int max_len) {
    return order >= 1 && order <= AR_MAX_ORDER && context >= 2 && context <= AR_MAX_CONTEXT && max_len >= 1 && max_len <= AR_MAX_LEN;
}

inline bool ar_args_ok(const float* wav, long stride, int B, long n, const int* count, const int* start, const int* length, int K, int order,
                       int context, int max_len, const float* out, long out_stride, const int* filled) {
    return wav != nullptr && count != nullptr && start != nullptr && length != nullptr && out != nullptr && filled != nullptr && B >= 1 &&
           K >= 1 && n >= 1 && n < (1L << 31) && stride >= n && out_stride >= n && (long)B * K <= 0x7fffffffL &&
           ar_limits_ok(order, context, max_len);
}

}  // namespace

extern "C" int viai_ar_fill(const float* wav, const int* lengths, long stride, int B, long n, const int* count, const int* start,
                            const int* length, int K, int order, int context, int max_len, float* out, long out_stride, int* filled,
                            void* stream) {
    if (!ar_args_ok(wav, stride, B, n, count, start, length, K, order, context, max_len, out, out_stride, filled) ||
        (reinterpret_cast<uintptr_t>(wav) & 3) != 0 || (reinterpret_cast<uintptr_t>(out) & 3) != 0)
        return (int)hipErrorInvalidValue;
    static bool attr = false;
    if (!attr) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(ar_fill_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)ar_lds_bytes(AR_MAX_CONTEXT, AR_MAX_LEN));
        attr = true;
    }
    VIAI_LAUNCH(ar_fill_kernel, dim3((unsigned)((long)B * K)), dim3(AR_THREADS), ar_lds_bytes(context, max_len), (hipStream_t)stream, wav, lengths,
                stride, n, count, start, length, K, order, context, max_len, ar_big_doubles(context, max_len), out, out_stride, filled);
    return viai_launch_status();
}

// The same rule with plain loops, every pointer in HOST memory.
extern "C" int viai_ar_fill_host(const float* wav, const int* lengths, long stride, int B, long n, const int* count, const int* start,
                                 const int* length, int K, int order, int context, int max_len, float* out, long out_stride, int* filled) {
    if (!ar_args_ok(wav, stride, B, n, count, start, length, K, order, context, max_len, out, out_stride, filled))
        return (int)hipErrorInvalidValue;
    std::vector<double> x(context), F(context), Bk(context);
    std::vector<double> pred[2];
    pred[0].resize(AR_MAX_ORDER + max_len);
    pred[1].resize(AR_MAX_ORDER + max_len);
    for (int b = 0; b < B; ++b) {
        const float* xr = wav + (long)b * stride;
        const int cnt = count[b], listed = cnt < K ? (cnt < 0 ? 0 : cnt) : K;
        const long len = ar_row_len(lengths, b, n);
        for (int k = 0; k < K; ++k) {
            const ArGap g = ar_gap(start + (long)b * K, length + (long)b * K, k, listed, len, order, context, max_len);
            filled[(long)b * K + k] = g.code;
            if (g.code == AR_SKIPPED) continue;
            const long e = g.s + g.L;
            const long C[2] = {g.cl, g.cr};
            const int p[2] = {g.pl, g.pr};
            for (int s = 0; s < 2; ++s) {
                if (p[s] < 1) continue;
                double a[AR_COEF];
                for (long j = 0; j < C[s]; ++j) x[j] = ar_sample(s == 0 ? xr[g.lo + j] : xr[e + C[1] - 1 - j]);
                ar_fit_plain(x.data(), C[s], p[s], a, F.data(), Bk.data());
                double* P = pred[s].data() + AR_MAX_ORDER;
                for (int j = 1; j <= p[s]; ++j) P[-j] = x[C[s] - j];
                for (long i = 0; i < g.L; ++i) P[i] = ar_predict(a, p[s], P + i);
            }
            float* yr = out + (long)b * out_stride + g.s;
            const double* P0 = pred[0].data() + AR_MAX_ORDER;
            const double* P1 = pred[1].data() + AR_MAX_ORDER;
            for (long i = 0; i < g.L; ++i) yr[i] = ar_blend(g.code, i, g.L, p[0] >= 1 ? P0[i] : 0.0, p[1] >= 1 ? P1[g.L - 1 - i] : 0.0);
        }
    }
    return 0;
}

// The fit alone: x (C,) fp32 in HOST memory -> a[0 .. order] (a[0] = 1, zeros behind a[p]) and *p = min(order, C / 2).
extern "C" int viai_ar_fit_host(const float* x, int C, int order, double* a, int* p) {
    if (x == nullptr || a == nullptr || p == nullptr || C < 0 || C > AR_MAX_CONTEXT || order < 1 || order > AR_MAX_ORDER)
        return (int)hipErrorInvalidValue;
    const int pp = C / 2 < order ? C / 2 : order;
    std::vector<double> xd(C > 0 ? C : 1), F(C > 0 ? C : 1), Bk(C > 0 ? C : 1);
    double af[AR_COEF];
    for (int j = 0; j < C; ++j) xd[j] = ar_sample(x[j]);
    ar_fit_plain(xd.data(), C, pp, af, F.data(), Bk.data());
    for (int j = 0; j <= order; ++j) a[j] = j <= pp ? af[j] : 0.0;
    *p = pp;
    return 0;
}
