// The arithmetic of the Burg autoregressive gap fill (include/viai_hip.h, "short gaps"), written ONCE: the kernel of ar_fill.hip and the host
// mirrors viai_ar_fill_host / viai_ar_fit_host call these same functions, so the same bits on the host and on the device are a property of
// the source.  fp64 throughout; only + - * /, each rounded once: contraction is off for everything below this line, hipcc's fp64 divide is the
// correctly rounded one (no fast-math flag in the Makefile), and no libm function is used.
//
// THE ORDER OF EVERY SUM IS PART OF THE RULE.
//   dot products of the fit (ar_dot3 states them with plain loops): AR_PARTS = 256 strided partials, partial t the terms i = t, t + 256,
//       t + 512, ... added in ascending i from +0.0 (acc = acc + x * y, two roundings); then the ADJACENT pairwise tree ar_tree: for o = 1, 2,
//       4, ... : p[t] = p[t] + p[t + o] for every t that is a multiple of 2 o.  On the device partial t is thread t's, the stages o < 64 are
//       the cross-lane stages of a wave64 and the last two are (w0 + w1) + (w2 + w3) over the four waves.
//   the p-term sum of one extrapolation step (ar_predict): AR_LANES = 64 partials, partial l the terms j = l + 1 and l + 65 (those that are
//       <= p, in that order), +0.0 for a lane without a term; then the same tree over 64; the new sample is 0.0 - sum.
#pragma once
#pragma clang fp contract(off)

#define AR_HD __host__ __device__ inline

#define AR_PARTS 256
#define AR_LANES 64
#define AR_MAX_ORDER 128
#define AR_MAX_CONTEXT 4096
#define AR_MAX_LEN 4096

// filled codes
#define AR_SKIPPED 0
#define AR_BOTH 1
#define AR_LEFT 2
#define AR_RIGHT 3
#define AR_NONE 4

// a context sample as the fit sees it: fp64, a non-finite one reads as 0.0
AR_HD double ar_sample(float x) { return (__builtin_bit_cast(unsigned, x) & 0x7fffffffu) < 0x7f800000u ? (double)x : 0.0; }

// 1. where gap k of a row lies and what it may read.  All positions are samples of the row; 64-bit so that no sum of two ints wraps.
struct ArGap {
    int code;           // AR_SKIPPED or the filled code the gap will get
    long s, L;          // the gap [s, s + L)
    long lo, cl;        // left context [lo, lo + cl), lo + cl == s
    long cr;            // right context [s + L, s + L + cr)
    int pl, pr;         // model orders of the two sides; 0: the side is not usable
};
AR_HD long ar_row_len(const int* lengths, int b, long n) {
    long len = lengths != nullptr ? (long)lengths[b] : n;
    len = len < 0 ? 0 : len;
    return len > n ? n : len;
}
// listed = min(count[b], K); start / length: the row's K entries
AR_HD ArGap ar_gap(const int* start, const int* length, int k, int listed, long len, int order, int context, int max_len) {
    ArGap g;
    g.code = AR_SKIPPED;
    g.s = g.L = g.lo = g.cl = g.cr = 0;
    g.pl = g.pr = 0;
    if (k >= listed) return g;
    const long s = start[k], L = length[k], e = s + L;
    if (L < 1 || L > max_len || s < 0 || e > len) return g;
    long lo = s - context;
    if (lo < 0) lo = 0;
    if (k > 0) {
        const long pe = (long)start[k - 1] + (long)length[k - 1];
        if (pe > lo) lo = pe;
    }
    long hi = e + context;
    if (hi > len) hi = len;
    if (k + 1 < listed) {
        const long ns = start[k + 1];
        if (ns < hi) hi = ns;
    }
    g.s = s;
    g.L = L;
    g.cl = s - lo > 0 ? s - lo : 0;
    g.lo = s - g.cl;
    g.cr = hi - e > 0 ? hi - e : 0;
    g.pl = (int)(g.cl / 2 < order ? g.cl / 2 : order);
    g.pr = (int)(g.cr / 2 < order ? g.cr / 2 : order);
    g.code = g.pl >= 1 ? (g.pr >= 1 ? AR_BOTH : AR_LEFT) : (g.pr >= 1 ? AR_RIGHT : AR_NONE);
    return g;
}

// 2. the pieces of one Burg stage
AR_HD double ar_mac(double acc, double x, double y) { return acc + x * y; }
AR_HD double ar_reflection(double fb, double ff, double bb) {
    const double den = ff + bb;
    return den == 0.0 ? 0.0 : (-2.0 * fb) / den;
}
AR_HD double ar_axpy(double x, double k, double y) { return x + k * y; }            // f' = f + k b, b' = b + k f, a'_j = a_j + k a_{m+1-j}
AR_HD double ar_sum4(double w0, double w1, double w2, double w3) { return (w0 + w1) + (w2 + w3); }

// the adjacent pairwise tree over p[0 .. n), n a power of two; the sum is left in p[0]
AR_HD double ar_tree(double* p, int n) {
    for (int o = 1; o < n; o *= 2)
        for (int t = 0; t < n; t += 2 * o) p[t] = p[t] + p[t + o];
    return p[0];
}

// the three dot products of stage m (0-based) in the rule's order, with plain loops: f_m[i] = F[i + m + 1], b_m[i] = B[i], i < C - 1 - m
AR_HD void ar_dot3(const double* F, const double* B, long C, int m, double* fb, double* ff, double* bb) {
    double pfb[AR_PARTS], pff[AR_PARTS], pbb[AR_PARTS];
    const long cnt = C - 1 - m;
    for (int t = 0; t < AR_PARTS; ++t) {
        double xfb = 0.0, xff = 0.0, xbb = 0.0;
        for (long i = t; i < cnt; i += AR_PARTS) {
            const double f = F[i + m + 1], b = B[i];
            xfb = ar_mac(xfb, f, b);
            xff = ar_mac(xff, f, f);
            xbb = ar_mac(xbb, b, b);
        }
        pfb[t] = xfb;
        pff[t] = xff;
        pbb[t] = xbb;
    }
    *fb = ar_tree(pfb, AR_PARTS);
    *ff = ar_tree(pff, AR_PARTS);
    *bb = ar_tree(pbb, AR_PARTS);
}

// 3. one extrapolation step.  lane l's partial: hist points at the sample to predict, hist[-j] is the sample j steps back
AR_HD double ar_term2(bool has1, double a1, double x1, bool has2, double a2, double x2) {
    double v = 0.0;
    if (has1) v = a1 * x1;
    if (has2) v = v + a2 * x2;
    return v;
}
AR_HD double ar_lane_term(const double* a, int p, const double* hist, int l) {
    const int j1 = l + 1, j2 = l + 1 + AR_LANES;
    const bool h1 = j1 <= p, h2 = j2 <= p;
    return ar_term2(h1, h1 ? a[j1] : 0.0, h1 ? hist[-j1] : 0.0, h2, h2 ? a[j2] : 0.0, h2 ? hist[-j2] : 0.0);
}
AR_HD double ar_step_value(double sum) { return 0.0 - sum; }
AR_HD double ar_predict(const double* a, int p, const double* hist) {
    double part[AR_LANES];
    for (int l = 0; l < AR_LANES; ++l) part[l] = ar_lane_term(a, p, hist, l);
    return ar_step_value(ar_tree(part, AR_LANES));
}

// 4. the cross-fade at sample i of a gap of L, rounded to fp32 once
AR_HD float ar_blend(int code, long i, long L, double fwd, double bwd) {
    if (code == AR_LEFT) return (float)fwd;
    if (code == AR_RIGHT) return (float)bwd;
    if (code != AR_BOTH) return 0.f;
    const double u = ((double)i + 0.5) / (double)L;
    const double t = (u * u) * (3.0 - 2.0 * u);
    const double w = 1.0 - t;
    return (float)(w * fwd + (1.0 - w) * bwd);
}
