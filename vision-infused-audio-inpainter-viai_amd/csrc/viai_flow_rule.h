// The per-pixel arithmetic of the TV-L1 optical flow (include/viai_hip.h, "optical flow"), written ONCE: the kernels of optical_flow.hip and
// the host mirror viai_optical_flow_host call these same functions, so the same bits on the host and on the device are a property of the
// source.  fp32 only; + - * / and sqrt, each rounded once: contraction is off for everything below this line, hipcc's divide and sqrt are the
// correctly rounded ones (no fast-math flag in the Makefile), and no libm function with an implementation-defined result is used (rintf is
// round-half-even on both sides).
#pragma once
#pragma clang fp contract(off)

#define FL_HD __host__ __device__ inline

// 1. grey: OpenCV's 8-bit BT.601 in int32
FL_HD float fl_grey(int r, int g, int b) { return (float)((4899 * r + 9617 * g + 1868 * b + 8192) >> 14); }

// 2. one pass of the 5-tap binomial (1 4 6 4 1) / 16: the products summed left to right
FL_HD float fl_binom5(float a, float b, float c, float d, float e) {
    return (((0.0625f * a + 0.25f * b) + 0.375f * c) + 0.25f * d) + 0.0625f * e;
}
FL_HD int fl_clampi(int v, int n) { return v < 0 ? 0 : (v > n - 1 ? n - 1 : v); }
// level k + 1 at (y, x) from level k (h x w): rows first (the five taps along x on each of five rows), then the five row results along y
FL_HD float fl_down(const float* src, int h, int w, int y, int x) {
    float r[5];
    for (int j = 0; j < 5; ++j) {
        const float* row = src + (long)fl_clampi(2 * y - 2 + j, h) * w;
        r[j] = fl_binom5(row[fl_clampi(2 * x - 2, w)], row[fl_clampi(2 * x - 1, w)], row[fl_clampi(2 * x, w)], row[fl_clampi(2 * x + 1, w)],
                         row[fl_clampi(2 * x + 2, w)]);
    }
    return fl_binom5(r[0], r[1], r[2], r[3], r[4]);
}

// a bilinear tap pair along one axis of n samples: the coordinate is clamped to [0, n - 1] BEFORE the floor, a NaN lands on 0, and the
// indices are formed from the clamped value only
struct FlTap { int i0, i1; float a; };
FL_HD FlTap fl_tap(float c, int n) {
    const float hi = (float)(n - 1);
    c = !(c >= 0.f) ? 0.f : (c > hi ? hi : c);
    FlTap t;
    t.i0 = (int)c;
    t.i1 = t.i0 + 1 < n ? t.i0 + 1 : n - 1;
    t.a = c - (float)t.i0;
    return t;
}
FL_HD float fl_lerp2(float v00, float v01, float v10, float v11, float ax, float ay) {
    const float bx = 1.f - ax, by = 1.f - ay;
    const float top = bx * v00 + ax * v01, bot = bx * v10 + ax * v11;
    return by * top + ay * bot;
}
// central differences with clamped indices, times 0.5
FL_HD float fl_dx(const float* I, int w, int y, int x) { return 0.5f * (I[(long)y * w + (x + 1 < w ? x + 1 : w - 1)] - I[(long)y * w + (x > 0 ? x - 1 : 0)]); }
FL_HD float fl_dy(const float* I, int h, int w, int y, int x) { return 0.5f * (I[(long)(y + 1 < h ? y + 1 : h - 1) * w + x] - I[(long)(y > 0 ? y - 1 : 0) * w + x]); }

// 3. coarse (hc x wc) to fine: u_f[y][x] = 2 bilinear(u_c, (x + 0.5) / 2 - 0.5, (y + 0.5) / 2 - 0.5)
FL_HD float fl_up(const float* uc, int hc, int wc, int y, int x) {
    const FlTap tx = fl_tap(((float)x + 0.5f) / 2.f - 0.5f, wc), ty = fl_tap(((float)y + 0.5f) / 2.f - 0.5f, hc);
    return 2.f * fl_lerp2(uc[(long)ty.i0 * wc + tx.i0], uc[(long)ty.i0 * wc + tx.i1], uc[(long)ty.i1 * wc + tx.i0], uc[(long)ty.i1 * wc + tx.i1],
                          tx.a, ty.a);
}

// 4. the warp at pixel (y, x) with flow (u, v): I1, I1x, I1y sampled bilinearly at (x + u, y + v)
struct FlWarp { float wx, wy, grad, rhoc; };
FL_HD FlWarp fl_warp(const float* I0, const float* I1, int h, int w, int y, int x, float u, float v) {
    const FlTap tx = fl_tap((float)x + u, w), ty = fl_tap((float)y + v, h);
    const float i1w = fl_lerp2(I1[(long)ty.i0 * w + tx.i0], I1[(long)ty.i0 * w + tx.i1], I1[(long)ty.i1 * w + tx.i0], I1[(long)ty.i1 * w + tx.i1],
                               tx.a, ty.a);
    FlWarp r;
    r.wx = fl_lerp2(fl_dx(I1, w, ty.i0, tx.i0), fl_dx(I1, w, ty.i0, tx.i1), fl_dx(I1, w, ty.i1, tx.i0), fl_dx(I1, w, ty.i1, tx.i1), tx.a, ty.a);
    r.wy = fl_lerp2(fl_dy(I1, h, w, ty.i0, tx.i0), fl_dy(I1, h, w, ty.i0, tx.i1), fl_dy(I1, h, w, ty.i1, tx.i0), fl_dy(I1, h, w, ty.i1, tx.i1),
                    tx.a, ty.a);
    r.grad = r.wx * r.wx + r.wy * r.wy;
    r.rhoc = ((i1w - r.wx * u) - r.wy * v) - I0[(long)y * w + x];
    return r;
}

// 5. one iteration, first half: the new (u, v) of a pixel from its constants, its old (u, v) and the two divergences
FL_HD void fl_step_u(float lt, float theta, const FlWarp& c, float div_u, float div_v, float* u, float* v) {
    const float rho = (c.rhoc + c.wx * *u) + c.wy * *v;
    const float thr = lt * c.grad;
    float du = 0.f, dv = 0.f;
    if (rho < -thr) {
        du = lt * c.wx; dv = lt * c.wy;
    } else if (rho > thr) {
        du = -(lt * c.wx); dv = -(lt * c.wy);
    } else if (c.grad > 1e-10f) {
        const float f = -rho / c.grad;
        du = f * c.wx; dv = f * c.wy;
    }
    *u = (*u + du) + theta * div_u;
    *v = (*v + dv) + theta * div_v;
}
// backward difference of a dual component along an axis of n samples at index i: pc = p[i], pl = p[i - 1] (not read for i == 0)
FL_HD float fl_bdiff(float pc, float pl, int i, int n) { return n == 1 ? 0.f : (i == 0 ? pc : (i == n - 1 ? -pl : pc - pl)); }
// second half: the dual pair of one component from the forward differences (gx, gy) of its NEW primal
FL_HD void fl_step_p(float taut, float gx, float gy, float* p1, float* p2) {
    const float den = 1.f + taut * __builtin_sqrtf(gx * gx + gy * gy);
    *p1 = (*p1 + taut * gx) / den;
    *p2 = (*p2 + taut * gy) / den;
}

// 6. the 8-bit encoding; a NaN encodes as 0 (the first test is written so that it takes it)
FL_HD unsigned char fl_encode(float f, float bound) {
    if (!(f >= -bound)) return 0;
    if (f > bound) return 255;
    const int q = (int)__builtin_rintf(255.f * (f + bound) / (2.f * bound));
    return (unsigned char)(q > 255 ? 255 : q);
}
