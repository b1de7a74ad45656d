// Burg's fit of viai_ar_rule.h as a block of 256 threads runs it, and the same fit in plain loops: shared by ar_fill.hip (two sides of a gap
// fitted together) and click_detect.hip (one tile).  The arithmetic and the order of every sum are the rule header's; nothing here adds any.
//
// ar_burg_block<NS>: NS recursions run TOGETHER, stage by stage.  Thread t owns the pairs (F[i + m + 1], B[i]), i = t, t + 256, ... of stage m, so
// its partial of each dot product is partial t of the rule and the elementwise update touches nothing another thread owns in that pass; the
// tree is four DPP stages and four readlanes per wave (wave_sum_d_dpp: the adjacent pairwise tree of the rule) and (w0 + w1) + (w2 + w3) over
// the waves (ar_sum4).  Two barriers per stage; every thread of the block must call it, and a barrier must stand between the staging of F, B,
// coef[..][0][0] = 1.0 and the call.
#pragma once
#include "viai_common.h"
#include "viai_ar_rule.h"

#pragma clang fp contract(off)

namespace {

constexpr int AR_THREADS = AR_PARTS;
constexpr int AR_COEF = AR_MAX_ORDER + 1;                       // a_0 .. a_128
static_assert(AR_THREADS == 256 && AR_LANES == 64, "four waves of 64: the tree of the rule");
static_assert(AR_COEF <= AR_THREADS && 2 * AR_MAX_ORDER <= AR_THREADS, "one thread per coefficient and per seed");

// LDS doubles behind the F / B arrays of a block that fits NS sides: coef[side][buffer][AR_COEF], red[wave][3 NS]
constexpr int ar_small_doubles(int ns) { return ns * 2 * AR_COEF + 4 * 3 * ns; }

// side s: F = fb + s * side_stride, B = F + b_off; C[s] samples, p[s] stages (0: the side is not fitted).  On return cur[s] names the buffer of
// coef that holds a[0 .. p[s]] (cur must come in as zeros), and F, B hold the last stage's errors.
template <int NS>
__device__ __forceinline__ void ar_burg_block(double* fb, long side_stride, long b_off, const long (&C)[NS], const int (&p)[NS], double* coef,
                                              double* red, int (&cur)[NS]) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int pmax = p[0];
    for (int s = 1; s < NS; ++s) pmax = p[s] > pmax ? p[s] : pmax;
    for (int m = 0; m < pmax; ++m) {
        double v[3 * NS];
#pragma unroll
        for (int q = 0; q < 3 * NS; ++q) v[q] = 0.0;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            if (m >= p[s]) continue;
            const double* F = fb + (long)s * side_stride;
            const double* B = F + b_off;
            const long pairs = C[s] - 1 - m;
            for (long i = tid; i < pairs; i += AR_THREADS) {
                const double f = F[i + m + 1], bk = B[i];
                v[3 * s] = ar_mac(v[3 * s], f, bk);
                v[3 * s + 1] = ar_mac(v[3 * s + 1], f, f);
                v[3 * s + 2] = ar_mac(v[3 * s + 2], bk, bk);
            }
        }
#pragma unroll
        for (int q = 0; q < 3 * NS; ++q) {
            const double w = wave_sum_d_dpp(v[q]);                            // every lane of every wave is here
            if (lane == 0) red[wv * 3 * NS + q] = w;
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            if (m >= p[s]) continue;
            const int W = 3 * NS;
            const double fb_ = ar_sum4(red[3 * s], red[W + 3 * s], red[2 * W + 3 * s], red[3 * W + 3 * s]);
            const double ff = ar_sum4(red[3 * s + 1], red[W + 3 * s + 1], red[2 * W + 3 * s + 1], red[3 * W + 3 * s + 1]);
            const double bb = ar_sum4(red[3 * s + 2], red[W + 3 * s + 2], red[2 * W + 3 * s + 2], red[3 * W + 3 * s + 2]);
            const double kr = ar_reflection(fb_, ff, bb);
            const double* a_old = coef + (s * 2 + cur[s]) * AR_COEF;
            double* a_new = coef + (s * 2 + (cur[s] ^ 1)) * AR_COEF;
            if (tid <= m + 1) {                                               // a <- [a, 0] + k reverse([a, 0])
                const double aj = tid <= m ? a_old[tid] : 0.0, ar = tid >= 1 ? a_old[m + 1 - tid] : 0.0;
                a_new[tid] = ar_axpy(aj, kr, ar);
            }
            cur[s] ^= 1;
            double* F = fb + (long)s * side_stride;
            double* B = F + b_off;
            const long pairs = C[s] - 1 - m;
            for (long i = tid; i < pairs; i += AR_THREADS) {
                const double f = F[i + m + 1], bk = B[i];
                F[i + m + 1] = ar_axpy(f, kr, bk);
                B[i] = ar_axpy(bk, kr, f);
            }
        }
        __syncthreads();
    }
}

// Burg on x[0 .. C) in plain loops: a[0 .. p], p = min(order, C / 2); F and B are scratch of C doubles each
inline void ar_fit_plain(const double* x, long C, int p, double* a, double* F, double* B) {
    double a_new[AR_COEF];
    for (long j = 0; j < C; ++j) F[j] = B[j] = x[j];
    a[0] = 1.0;
    for (int m = 0; m < p; ++m) {
        double fb, ff, bb;
        ar_dot3(F, B, C, m, &fb, &ff, &bb);
        const double kr = ar_reflection(fb, ff, bb);
        for (int j = 0; j <= m + 1; ++j) a_new[j] = ar_axpy(j <= m ? a[j] : 0.0, kr, j >= 1 ? a[m + 1 - j] : 0.0);
        for (int j = 0; j <= m + 1; ++j) a[j] = a_new[j];
        for (long i = 0; i < C - 1 - m; ++i) {
            const double f = F[i + m + 1], bk = B[i];
            F[i + m + 1] = ar_axpy(f, kr, bk);
            B[i] = ar_axpy(bk, kr, f);
        }
    }
}

}  // namespace
