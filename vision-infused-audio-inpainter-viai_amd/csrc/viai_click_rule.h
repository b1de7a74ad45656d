// The arithmetic of the click detector (include/viai_hip.h, "clicks"), written ONCE: the kernels of click_detect.hip and the host mirror
// viai_click_detect_host call these same functions, so the same flags on the host and on the device are a property of the source.  fp64
// throughout; only + - * / and comparisons, each operation rounded once (contraction is off below this line); no sqrt, no median, no libm.
// The fit is Burg's of viai_ar_rule.h, unchanged: 256 strided partials, the adjacent pairwise tree, ar_reflection, ar_axpy.
//
// THE ORDER OF EVERY SUM IS PART OF THE RULE.
//   residual of sample g (cd_residual states it): e = sum_{j = 0 .. p} a[j] xs(g - j), from +0.0 in ascending j, acc = acc + a x (two roundings)
//   sum of the squared residuals of a tile, and of those under the cut: the fit's dot-product order.  CD_PARTS = 256 strided partials, partial
//       t the tile-local indices i = t, t + 256, ... in ascending i from +0.0 (acc = acc + q, samples that are not judged or lie above the
//       cut are left out, not added as zeros), then ar_tree over 256.  On the device partial t is thread t's.
#pragma once
#include "viai_ar_rule.h"

#pragma clang fp contract(off)

#define CD_PARTS AR_PARTS
#define CD_MAX_PASSES 4
#define CD_MAX_GUARD 64

// k and floor arrive as fp32; the rule squares them in fp64
AR_HD double cd_square(float v) { return (double)v * (double)v; }

// the model order of a tile of C samples
AR_HD int cd_order(int order, long C) { return (int)(C / 2 < order ? C / 2 : order); }

// the prediction error at x[0]: x points at sample g of the row, x[-j] is the sample j steps back (g >= p, so all of them exist)
AR_HD double cd_residual(const double* a, int p, const float* x) {
    double acc = 0.0;
    for (int j = 0; j <= p; ++j) acc = ar_mac(acc, a[j], ar_sample(x[-j]));
    return acc;
}

// one more term of a partial
AR_HD double cd_add(double acc, double q) { return acc + q; }

// the scale after a pass: the mean of the kept squares; no kept sample leaves it as it was
AR_HD double cd_mean(double sum, long cnt, double var) { return cnt > 0 ? sum / (double)cnt : var; }

// a sample stays in the next pass's mean
AR_HD bool cd_keep(double q, double kk, double var) { return q <= kk * var; }

// a judged sample is a click
AR_HD bool cd_flag(double q, double kk, double var, double ff) { return q > kk * (var > ff ? var : ff); }

// a sample that is flagged whatever the model says
AR_HD bool cd_nonfinite(float x) { return (__builtin_bit_cast(unsigned, x) & 0x7fffffffu) >= 0x7f800000u; }
