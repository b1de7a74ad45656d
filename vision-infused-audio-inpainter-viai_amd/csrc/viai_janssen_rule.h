// The arithmetic of Janssen's least-squares AR interpolation (include/viai_hip.h, "crackle and short gaps"), written ONCE on top of
// viai_ar_rule.h: the kernel of janssen_fill.hip and the host mirrors viai_janssen_fill_host / viai_janssen_plan_host call these same
// functions, so the same bits on the host and on the device are a property of the source.  fp64 throughout; only + - * / and comparisons,
// each rounded once: contraction is off for everything below this line, and no libm function is used.
//
// THE ORDER OF EVERY SUM IS PART OF THE RULE.
//   the fit: Burg of viai_ar_rule.h on the whole window (256 strided partials and the adjacent pairwise tree), unchanged.
//   b_l (jn_autocorr): the terms k = 0, 1, ..., p - l in ascending k from +0.0, acc = acc + a_k * a_{k+l} (two roundings a term).  On the
//       device thread l owns b_l.
//   r_i (jn_rhs): the terms l = -p, ..., p in ascending l that fall inside the window, from +0.0, acc = acc + b_|l| * x0[t_i + l], where x0 is
//       the window with 0.0 at every unknown (so an unknown's term adds a zero and a known sample's term is the sum's); r_i = 0.0 - acc.  On the
//       device thread i mod 256 owns r_i.
//   L D L^T (jn_ldl_plain states it with plain loops): right-looking, column by column, inside the INDEX band of p sub-diagonals (unknowns i and
//       j with |i - j| <= p; |t_i - t_j| >= |i - j|, so every non-zero of G and all fill lies there).  At column j: d_j = A_jj; for i = j + 1 ..
//       min(j + p, M - 1): c_i = A_ij, l_i = c_i / d_j; then A_ik = A_ik - l_i * c_k for j < k <= i (one rounded product, one rounded
//       difference; l_i * c_k, NOT l_i * d_j * l_k).  Every element therefore takes its updates one at a time in ascending j, whether the
//       factor is zero or not.  The forward substitution rides along: z_i = z_i - l_i * z_j for the same i, ascending j.
//   y_i = z_i / d_i; back substitution column by column in DESCENDING j: x_i = x_i - l_ji * x_j for i = j - 1, ..., max(j - p, 0).
//   On the device every (i, k) of a column is one thread's, and the back substitution is one wave's, lane q the rows j - 1 - q and j - 65 - q.
#pragma once
#include "viai_ar_rule.h"

#pragma clang fp contract(off)

#define JN_MAX_UNKNOWN 1024
#define JN_BAND_DOUBLES 8192
#define JN_MAX_WINDOW 4096
#define JN_MAX_CONTEXT 1024
#define JN_MAX_ITERS 16

// filled codes (0 skipped and 4 no model are AR_SKIPPED and AR_NONE)
#define JN_SOLVED 1
#define JN_PIVOT 5

// the largest max_len the limits leave for one entry
AR_HD int jn_max_len(int order, int context) {
    int m = JN_MAX_UNKNOWN;
    if (JN_BAND_DOUBLES / (order + 1) < m) m = JN_BAND_DOUBLES / (order + 1);
    if (JN_MAX_WINDOW - 2 * context < m) m = JN_MAX_WINDOW - 2 * context;
    return m;
}

// 1. + 2. + 3.  the cluster of entry k of a row and its window.  Integers only; 64-bit so that no sum of two ints wraps.
//   front_i = max(0, start[j] + max(length[j], 0) over j < i): the end of everything listed in front of entry i.  For lists in position order it
//       is the end of entry i - 1; taking the running maximum keeps the promise "a window holds no unknown of another cluster" for ANY list.
//   usable   1 <= L <= max_len, s >= front_i, s + L <= len.
//   clusters a cluster opens at a usable entry that does not join; usable entry i joins the open cluster iff s_i - e_last < context,
//            M + L_i <= JN_MAX_UNKNOWN, (M + L_i)(order + 1) <= JN_BAND_DOUBLES and (e_i - s_first) + 2 context <= JN_MAX_WINDOW.  An entry that
//            is not usable closes the open cluster.
//   window   [max(s_first - context, front_first, 0), max(min(e_last + context, start of the entry behind the last member, len), e_last)).
struct JnPlan {
    int leader;         // index of the cluster's first member; -1: entry k is skipped
    int last;           // index of its last member
    long lo, hi;        // the window
    long M;             // its unknowns
};
AR_HD JnPlan jn_plan(const int* start, const int* length, int k, int listed, long len, int order, int context, int max_len) {
    JnPlan pl;
    pl.leader = -1;
    pl.last = -1;
    pl.lo = pl.hi = pl.M = 0;
    if (k >= listed) return pl;
    long front = 0, M = 0, sf = 0, el = 0, wl = 0, wr = 0;
    bool open = false, walled = false;
    int lead = 0, last = 0;
    for (int i = 0; i < listed; ++i) {
        const long s = start[i], L = length[i], e = s + L;
        const bool usable = L >= 1 && L <= max_len && s >= front && e <= len;
        const bool join = usable && open && s - el < context && M + L <= JN_MAX_UNKNOWN && (M + L) * (order + 1) <= JN_BAND_DOUBLES &&
                          (e - sf) + 2L * context <= JN_MAX_WINDOW;
        if (open && !join) {
            if (i > k) {                        // the cluster that holds k closes here: entry i is its right wall
                wr = s;
                walled = true;
                break;
            }
            open = false;
        }
        if (i == k && !usable) return pl;
        if (usable) {
            if (!join) {
                open = true;
                lead = i;
                sf = s;
                M = 0;
                wl = front;
            }
            M += L;
            el = e;
            last = i;
        }
        const long end = s + (L > 0 ? L : 0);
        if (end > front) front = end;
    }
    long lo = sf - context, hi = el + context;
    if (lo < wl) lo = wl;                       // wl >= 0
    if (hi > len) hi = len;
    if (walled && wr < hi) hi = wr;
    if (hi < el) hi = el;
    pl.leader = lead;
    pl.last = last;
    pl.lo = lo;
    pl.hi = hi;
    pl.M = M;
    return pl;
}

// 4. the pieces of one iteration
AR_HD double jn_autocorr(const double* a, int p, int l) {
    double acc = 0.0;
    for (int k = 0; k + l <= p; ++k) acc = ar_mac(acc, a[k], a[k + l]);
    return acc;
}
// x0: the window, 0.0 at the unknowns; t: the unknown's position in it
AR_HD double jn_rhs(const double* b, int p, const double* x0, long W, long t) {
    double acc = 0.0;
    for (int l = -p; l <= p; ++l) {
        const long q = t + l;
        if (q >= 0 && q < W) acc = ar_mac(acc, b[l < 0 ? -l : l], x0[q]);
    }
    return 0.0 - acc;
}
AR_HD double jn_gram(const double* b, int p, long dt) { return dt <= p ? b[dt] : 0.0; }
AR_HD bool jn_pivot_ok(double d) { return d > 0.0 && d <= 1.7976931348623157e308; }
AR_HD double jn_div(double c, double d) { return c / d; }
AR_HD double jn_down(double x, double l, double c) { return x - l * c; }

// the band: row i holds A_ij, j = i - p .. i, at band[i (p + 1) + (j - i + p)]; the slots of j < 0 are not used
AR_HD long jn_at(long i, long j, int p) { return i * (p + 1) + (j - i + p); }
AR_HD void jn_band_fill(double* band, const int* t, long M, int p, const double* b) {
    for (long i = 0; i < M; ++i)
        for (int c = 0; c <= p; ++c) {
            const long j = i - p + c;
            band[i * (p + 1) + c] = j < 0 ? 0.0 : jn_gram(b, p, (long)t[i] - (long)t[j]);
        }
}
// factor and solve in the rule's order with plain loops: z (M,) comes in as r and leaves as the solution; col is scratch of p doubles.
// false: column j's pivot is not > 0.0 or not finite, z is then of no use.
AR_HD bool jn_ldl_plain(double* band, long M, int p, double* z, double* col) {
    for (long j = 0; j < M; ++j) {
        const double d = band[jn_at(j, j, p)];
        if (!jn_pivot_ok(d)) return false;
        const long cnt = M - 1 - j < p ? M - 1 - j : p;
        for (long q = 0; q < cnt; ++q) {
            const long i = j + 1 + q;
            const double c = band[jn_at(i, j, p)], l = jn_div(c, d);
            col[q] = c;
            band[jn_at(i, j, p)] = l;
            z[i] = jn_down(z[i], l, z[j]);
        }
        for (long qi = 0; qi < cnt; ++qi)
            for (long qk = 0; qk <= qi; ++qk) {
                const long i = j + 1 + qi, k = j + 1 + qk;
                band[jn_at(i, k, p)] = jn_down(band[jn_at(i, k, p)], band[jn_at(i, j, p)], col[qk]);
            }
    }
    for (long i = 0; i < M; ++i) z[i] = jn_div(z[i], band[jn_at(i, i, p)]);
    for (long j = M - 1; j >= 0; --j) {
        const long cnt = j < p ? j : p;
        for (long q = 0; q < cnt; ++q) {
            const long i = j - 1 - q;
            z[i] = jn_down(z[i], band[jn_at(j, i, p)], z[j]);
        }
    }
    return true;
}
