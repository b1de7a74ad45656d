// The arithmetic of bound-constrained Janssen restoration of clipped samples (include/viai_hip.h, "declipping"), written ONCE on top of
// viai_janssen_rule.h and viai_ar_rule.h: the kernel of declip.hip and the host mirror viai_declip_host call these same functions, so the same
// bits on the host and on the device are a property of the source.  fp64 throughout; only + - * / and comparisons, each rounded once:
// contraction is off for everything below this line, and no libm function is used.
//
// THE ORDER OF EVERY SUM IS PART OF THE RULE, and every sum here is one of the Janssen rule's:
//   the fit, b_l (jn_autocorr), L D L^T with its forward and back substitution (jn_ldl_plain): unchanged.
//   r_i (jn_rhs): the same ascending l = -p .. p from +0.0 over x0, where x0 now holds 0.0 at the FREE unknowns and c_i at the PINNED ones, so a
//       pinned unknown's term is a known sample's term.
//   the band of a re-solve (dc_band_fill): the Gram band of the free unknowns alone, taken in position order; element (i, j) is
//       b_|t_f(i) - t_f(j)| inside p, else 0.0.  No sum.
//   the compaction f(0) < f(1) < ... of the free unknowns is an exclusive count in position order: integers only.
// What this is NOT: an exact quadratic program.  Pins are never released within an iteration (an active-set heuristic without release), and
// the final clamp is a projection, not a solve.
#pragma once
#include "viai_janssen_rule.h"

#pragma clang fp contract(off)

#define DC_MAX_ROUNDS 8

// BOUND.  c = ar_sample(ref[t]): c > 0 asks x >= c, c < 0 asks x <= c, c == 0 (a dropout, a non-finite sample) asks nothing.  Written so that a
// NaN estimate violates a bound that is there.
AR_HD bool dc_violates(double c, double x) { return c > 0.0 ? !(x >= c) : (c < 0.0 ? !(x <= c) : false); }

// USABLE and CLUSTERS are jn_plan's; the WINDOW is [max(s_first - context, 0), min(e_last + context, len)): NOT cut at neighbouring entries.  The
// cluster rule bounds it: (e_last - s_first) + 2 context <= JN_MAX_WINDOW.
AR_HD JnPlan dc_plan(const int* start, const int* length, int k, int listed, long len, int order, int context, int max_len) {
    JnPlan pl = jn_plan(start, length, k, listed, len, order, context, max_len);
    if (pl.leader < 0) return pl;
    long lo = (long)start[pl.leader] - context, hi = (long)start[pl.last] + (long)length[pl.last] + context;
    if (lo < 0) lo = 0;
    if (hi > len) hi = len;                     // a usable entry ends at or before len, so hi >= e_last
    pl.lo = lo;
    pl.hi = hi;
    return pl;
}

// the pin bitmap: bit i & 63 of word i >> 6
AR_HD bool dc_pinned(const unsigned long long* pin, int i) { return ((pin[i >> 6] >> (i & 63)) & 1ull) != 0; }

// the band of the free unknowns f[0 .. Mf) (indices into t, ascending); f == nullptr: all of t
AR_HD int dc_pos(const int* t, const int* f, long i) { return f != nullptr ? t[f[i]] : t[i]; }
AR_HD void dc_band_fill(double* band, const int* t, const int* f, long Mf, int p, const double* b) {
    for (long i = 0; i < Mf; ++i)
        for (int c = 0; c <= p; ++c) {
            const long j = i - p + c;
            band[i * (p + 1) + c] = j < 0 ? 0.0 : jn_gram(b, p, (long)dc_pos(t, f, i) - (long)dc_pos(t, f, j));
        }
}
