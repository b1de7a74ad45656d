// TV-L1 optical flow (gfx950): raw uint8 frames in, fp32 flow and the dataset's 8-bit flow maps out.
// Contract and rule: include/viai_hip.h; the per-pixel arithmetic: viai_flow_rule.h (shared with the host mirror); launches, bytes moved and
// measured rates: DESIGN.md 11.2o.
//
//   fl_grey_kernel    frames -> level 0 of the pyramid of every frame of the call
//   fl_down_kernel    level k -> level k + 1 (25 taps per output pixel)
//   fl_warp_kernel    the four constants of a warp (I1wx, I1wy, grad, rho_c) per pixel and pair; at the coarsest level's first warp it also
//                     writes u = v = 0
//   fl_iter_kernel    k <= 8 iterations in one launch.  A block owns a 32 x 32 tile, stages the six evolving planes of the tile plus a halo of k
//                     (cut at the image border) in LDS, keeps the four constants of its pixels in registers, and runs the k iterations over a
//                     rectangle that loses one column / row per half step on every side that is not the image border: after k iterations exactly
//                     the tile is left, and every value in it went through the operations of the plain form.  Reads one state buffer, writes the
//                     other: blocks never see each other's results within a launch.
//   fl_up_kernel      (u, v) of a level -> the next finer level
//   fl_store_kernel   (u, v) of level 0 -> flow (pairs, 2, H, W)
//   fl_encode_kernel  flow -> the two uint8 stacks
// Pair = grid z in every kernel, so the launch count does not depend on the number of frames.
#include <vector>

#include "viai_common.h"
#include "viai_internal.h"
#include "viai_flow_rule.h"

namespace {

constexpr int FL_TW = VIAI_FLOW_TILE_W, FL_TH = VIAI_FLOW_TILE_H, FL_KMAX = VIAI_FLOW_MAX_ITERS_PER_LAUNCH;
constexpr int FL_THREADS = 256;
constexpr int FL_RMAX = (FL_TW + 2 * FL_KMAX) * (FL_TH + 2 * FL_KMAX);          // pixels of the largest staged region
constexpr int FL_PER = (FL_RMAX + FL_THREADS - 1) / FL_THREADS;                  // pixels of a thread
constexpr int FL_MAX_DIM = 1 << 15;
constexpr int FL_MAX_LEVELS = 12;                                                // 2^15 / 2^11 = 16: no more levels can have 16 samples
constexpr int FL_MAX_PAIRS = 65535;                                              // grid z
static_assert(6 * FL_RMAX * 4 <= 64 * 1024, "the six staged planes fit the 64 KiB a block may declare");

struct FlLevels {
    int S, h[FL_MAX_LEVELS], w[FL_MAX_LEVELS];
    long off[FL_MAX_LEVELS], total;                                              // floats of one frame's pyramid
};

inline FlLevels fl_levels(int H, int W, int scales) {
    FlLevels L;
    L.S = 1; L.h[0] = H; L.w[0] = W; L.off[0] = 0; L.total = (long)H * W;
    while (L.S < scales && L.S < FL_MAX_LEVELS) {
        const int h = (L.h[L.S - 1] + 1) / 2, w = (L.w[L.S - 1] + 1) / 2;
        if (h < 16 || w < 16) break;
        L.h[L.S] = h; L.w[L.S] = w; L.off[L.S] = L.total; L.total += (long)h * w; ++L.S;
    }
    return L;
}

inline bool fl_pos(float v) { return v > 0.f; }                                  // false for a NaN

bool fl_args_ok(const void* frames, long fstride, int N, int H, int W, int C, float tau, float lam, float theta, int scales, int warps,
                int iterations, int ipl, const void* flow) {
    if (frames == nullptr || flow == nullptr || N < 2 || N - 1 > FL_MAX_PAIRS) return false;
    if (H < 1 || W < 1 || H >= FL_MAX_DIM || W >= FL_MAX_DIM || (C != 1 && C != 3 && C != 4) || fstride < (long)H * W * C) return false;
    if (scales < 1 || warps < 1 || iterations < 1 || ipl < 1 || ipl > FL_KMAX) return false;
    return fl_pos(tau) && fl_pos(lam) && fl_pos(theta);
}

inline dim3 fl_grid(int h, int w, int z) { return dim3((unsigned)((w + 63) / 64), (unsigned)((h + 3) / 4), (unsigned)z); }   // 64 x 4 pixels

// the pixel of a streaming kernel's thread
#define FL_PIXEL(h, w)                                                   \
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6), z = blockIdx.z; \
    if (x >= (w) || y >= (h)) return

__global__ __launch_bounds__(FL_THREADS) void fl_grey_kernel(const unsigned char* __restrict__ frames, long fstride, int C, int ro, int bo, int H,
                                                             int W, float* __restrict__ pyr, long total) {
    FL_PIXEL(H, W);
    const unsigned char* p = frames + (long)z * fstride + ((long)y * W + x) * C;
    pyr[(long)z * total + (long)y * W + x] = C == 1 ? (float)p[0] : fl_grey(p[ro], p[1], p[bo]);
}

__global__ __launch_bounds__(FL_THREADS) void fl_down_kernel(float* __restrict__ pyr, long total, long off_s, int hs, int ws, long off_d, int hd,
                                                             int wd) {
    FL_PIXEL(hd, wd);
    float* f = pyr + (long)z * total;
    f[off_d + (long)y * wd + x] = fl_down(f + off_s, hs, ws, y, x);
}

// state and constants: plane j of pair z at base + (j * P + z) * HW0, whatever the level
__global__ __launch_bounds__(FL_THREADS) void fl_warp_kernel(const float* __restrict__ pyr, long total, long off, int h, int w, int P, long HW0,
                                                             float* __restrict__ st, float* __restrict__ cst, int zero) {
    FL_PIXEL(h, w);
    const long at = (long)z * HW0 + (long)y * w + x, pl = (long)P * HW0;
    float u = 0.f, v = 0.f;
    if (zero) { st[at] = 0.f; st[pl + at] = 0.f; }
    else { u = st[at]; v = st[pl + at]; }
    const FlWarp r = fl_warp(pyr + (long)z * total + off, pyr + (long)(z + 1) * total + off, h, w, y, x, u, v);
    cst[at] = r.wx; cst[pl + at] = r.wy; cst[2 * pl + at] = r.grad; cst[3 * pl + at] = r.rhoc;
}

__global__ __launch_bounds__(FL_THREADS) void fl_iter_kernel(const float* __restrict__ sin, float* __restrict__ sout, const float* __restrict__ cst,
                                                             int P, long HW0, int h, int w, int k, int p_zero, float lt, float theta, float taut) {
    __shared__ float s[6][FL_RMAX];
    const int tid = threadIdx.x, z = blockIdx.z;
    const int tx0 = blockIdx.x * FL_TW, ty0 = blockIdx.y * FL_TH;
    const int tx1 = tx0 + FL_TW < w ? tx0 + FL_TW : w, ty1 = ty0 + FL_TH < h ? ty0 + FL_TH : h;
    // the staged region: the tile and a halo of k, cut at the image
    const int rx0 = tx0 - k > 0 ? tx0 - k : 0, ry0 = ty0 - k > 0 ? ty0 - k : 0;
    const int rx1 = tx1 + k < w ? tx1 + k : w, ry1 = ty1 + k < h ? ty1 + k : h;
    const int RW = rx1 - rx0, npx = RW * (ry1 - ry0);                            // <= FL_RMAX: k <= FL_KMAX is checked on the host
    const long pl = (long)P * HW0, zb = (long)z * HW0;

    FlWarp c[FL_PER];
    int X[FL_PER], Y[FL_PER];
#pragma unroll
    for (int j = 0; j < FL_PER; ++j) {
        const int i = tid + j * FL_THREADS;
        X[j] = Y[j] = -1;
        c[j].wx = c[j].wy = c[j].grad = c[j].rhoc = 0.f;
        if (i < npx) {
            const int ry = i / RW, rx = i - ry * RW;
            X[j] = rx0 + rx; Y[j] = ry0 + ry;
            const long at = zb + (long)Y[j] * w + X[j];
            s[0][i] = sin[at]; s[1][i] = sin[pl + at];
#pragma unroll
            for (int q = 2; q < 6; ++q) s[q][i] = p_zero ? 0.f : sin[q * pl + at];
            c[j].wx = cst[at]; c[j].wy = cst[pl + at]; c[j].grad = cst[2 * pl + at]; c[j].rhoc = cst[3 * pl + at];
        }
    }
    __syncthreads();

    int ax = rx0, bx = rx1, ay = ry0, by = ry1;                                  // where u, v and p are those of the plain form
    for (int it = 0; it < k; ++it) {
        // u, v: needs p at x - 1 and y - 1, so the left and top sides move in unless they are the image border
        ax = ax > 0 ? ax + 1 : 0; ay = ay > 0 ? ay + 1 : 0;
#pragma unroll
        for (int j = 0; j < FL_PER; ++j) {
            const int i = tid + j * FL_THREADS, x = X[j], y = Y[j];
            if (x >= ax && x < bx && y >= ay && y < by) {
                const float div_u = fl_bdiff(s[2][i], x > 0 ? s[2][i - 1] : 0.f, x, w) + fl_bdiff(s[3][i], y > 0 ? s[3][i - RW] : 0.f, y, h);
                const float div_v = fl_bdiff(s[4][i], x > 0 ? s[4][i - 1] : 0.f, x, w) + fl_bdiff(s[5][i], y > 0 ? s[5][i - RW] : 0.f, y, h);
                float u = s[0][i], v = s[1][i];
                fl_step_u(lt, theta, c[j], div_u, div_v, &u, &v);
                s[0][i] = u; s[1][i] = v;
            }
        }
        __syncthreads();
        // p: needs the new u, v at x + 1 and y + 1, so the right and bottom sides move in unless they are the image border
        bx = bx < w ? bx - 1 : w; by = by < h ? by - 1 : h;
#pragma unroll
        for (int j = 0; j < FL_PER; ++j) {
            const int i = tid + j * FL_THREADS, x = X[j], y = Y[j];
            if (x >= ax && x < bx && y >= ay && y < by) {
                const float u = s[0][i], v = s[1][i];
                const float ux = x < w - 1 ? s[0][i + 1] - u : 0.f, uy = y < h - 1 ? s[0][i + RW] - u : 0.f;
                const float vx = x < w - 1 ? s[1][i + 1] - v : 0.f, vy = y < h - 1 ? s[1][i + RW] - v : 0.f;
                fl_step_p(taut, ux, uy, &s[2][i], &s[3][i]);
                fl_step_p(taut, vx, vy, &s[4][i], &s[5][i]);
            }
        }
        __syncthreads();
    }
    // the rectangle left is the tile (or more, towards an image border); the tile is what this block owns
#pragma unroll
    for (int j = 0; j < FL_PER; ++j) {
        const int i = tid + j * FL_THREADS, x = X[j], y = Y[j];
        if (x >= tx0 && x < tx1 && y >= ty0 && y < ty1) {
            const long at = zb + (long)y * w + x;
#pragma unroll
            for (int q = 0; q < 6; ++q) sout[q * pl + at] = s[q][i];
        }
    }
}

__global__ __launch_bounds__(FL_THREADS) void fl_up_kernel(const float* __restrict__ sc, float* __restrict__ sf, int P, long HW0, int hc, int wc,
                                                           int h, int w) {
    FL_PIXEL(h, w);
    const long pl = (long)P * HW0, zb = (long)z * HW0;
    sf[zb + (long)y * w + x] = fl_up(sc + zb, hc, wc, y, x);
    sf[pl + zb + (long)y * w + x] = fl_up(sc + pl + zb, hc, wc, y, x);
}

__global__ __launch_bounds__(FL_THREADS) void fl_store_kernel(const float* __restrict__ st, int P, long HW0, int H, int W, float* __restrict__ flow) {
    FL_PIXEL(H, W);
    const long at = (long)y * W + x;
    flow[(2L * z) * HW0 + at] = st[(long)z * HW0 + at];
    flow[(2L * z + 1) * HW0 + at] = st[((long)P + z) * HW0 + at];
}

__global__ __launch_bounds__(FL_THREADS) void fl_encode_kernel(const float* __restrict__ flow, int pairs, long HW, float bound,
                                                               unsigned char* __restrict__ fx, unsigned char* __restrict__ fy) {
    const long i = blockIdx.x * (long)FL_THREADS + threadIdx.x;
    const int z = blockIdx.y, src = z < pairs ? z : pairs - 1;                   // grid y = maps written; the last repeats with pad_last
    if (i >= HW) return;
    fx[(long)z * HW + i] = fl_encode(flow[(2L * src) * HW + i], bound);
    fy[(long)z * HW + i] = fl_encode(flow[(2L * src + 1) * HW + i], bound);
}

bool fl_encode_args_ok(const void* flow, int pairs, int H, int W, float bound, const void* fx, const void* fy) {
    return flow != nullptr && fx != nullptr && fy != nullptr && pairs >= 1 && pairs <= FL_MAX_PAIRS - 1 && H >= 1 && W >= 1 && H < FL_MAX_DIM &&
           W < FL_MAX_DIM && fl_pos(bound);
}

}  // namespace

extern "C" int viai_optical_flow_levels(int H, int W, int scales) {
    if (H < 1 || W < 1 || H >= FL_MAX_DIM || W >= FL_MAX_DIM || scales < 1) return 0;
    return fl_levels(H, W, scales).S;
}

extern "C" long viai_optical_flow_ws_bytes(int pairs, int H, int W, int scales) {
    if (pairs < 1 || pairs > FL_MAX_PAIRS || H < 1 || W < 1 || H >= FL_MAX_DIM || W >= FL_MAX_DIM || scales < 1) return 0;
    const FlLevels L = fl_levels(H, W, scales);
    return (long)sizeof(float) * ((long)(pairs + 1) * L.total + 16L * pairs * H * W);
}

extern "C" int viai_optical_flow_launches(int H, int W, int scales, int warps, int iterations, int iters_per_launch) {
    if (H < 1 || W < 1 || H >= FL_MAX_DIM || W >= FL_MAX_DIM || scales < 1 || warps < 1 || iterations < 1 || iters_per_launch < 1 ||
        iters_per_launch > FL_KMAX)
        return 0;
    const int S = fl_levels(H, W, scales).S;
    return 1 + (S - 1) + S * warps * (1 + (iterations + iters_per_launch - 1) / iters_per_launch) + (S - 1) + 1;
}

extern "C" int viai_optical_flow(const unsigned char* frames, long frame_stride, int N, int H, int W, int C, int bgr, float tau, float lam,
                                 float theta, int scales, int warps, int iterations, int iters_per_launch, float* flow, void* ws, void* stream) {
    if (!fl_args_ok(frames, frame_stride, N, H, W, C, tau, lam, theta, scales, warps, iterations, iters_per_launch, flow) || ws == nullptr ||
        (reinterpret_cast<uintptr_t>(ws) & 3) != 0)
        return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    const FlLevels L = fl_levels(H, W, scales);
    const int P = N - 1;
    const long HW0 = (long)H * W;
    float* pyr = static_cast<float*>(ws);
    float* state[2] = {pyr + (long)N * L.total, pyr + (long)N * L.total + 6L * P * HW0};
    float* cst = state[1] + 6L * P * HW0;
    const float lt = lam * theta, taut = tau / theta;

    VIAI_LAUNCH(fl_grey_kernel, fl_grid(H, W, N), dim3(FL_THREADS), 0, st, frames, frame_stride, C, bgr ? 2 : 0, bgr ? 0 : 2, H, W, pyr, L.total);
    for (int l = 1; l < L.S; ++l)
        VIAI_LAUNCH(fl_down_kernel, fl_grid(L.h[l], L.w[l], N), dim3(FL_THREADS), 0, st, pyr, L.total, L.off[l - 1], L.h[l - 1], L.w[l - 1], L.off[l],
                    L.h[l], L.w[l]);
    int cur = 0;
    for (int l = L.S - 1; l >= 0; --l) {
        const int h = L.h[l], w = L.w[l];
        if (l < L.S - 1) {
            VIAI_LAUNCH(fl_up_kernel, fl_grid(h, w, P), dim3(FL_THREADS), 0, st, state[cur], state[cur ^ 1], P, HW0, L.h[l + 1], L.w[l + 1], h, w);
            cur ^= 1;
        }
        const dim3 tiles((unsigned)((w + FL_TW - 1) / FL_TW), (unsigned)((h + FL_TH - 1) / FL_TH), (unsigned)P);
        for (int wp = 0; wp < warps; ++wp) {
            VIAI_LAUNCH(fl_warp_kernel, fl_grid(h, w, P), dim3(FL_THREADS), 0, st, pyr, L.total, L.off[l], h, w, P, HW0, state[cur], cst,
                        (l == L.S - 1 && wp == 0) ? 1 : 0);
            for (int done = 0; done < iterations; done += iters_per_launch) {
                const int k = iterations - done < iters_per_launch ? iterations - done : iters_per_launch;
                VIAI_LAUNCH(fl_iter_kernel, tiles, dim3(FL_THREADS), 0, st, state[cur], state[cur ^ 1], cst, P, HW0, h, w, k,
                            (wp == 0 && done == 0) ? 1 : 0, lt, theta, taut);
                cur ^= 1;
            }
        }
    }
    VIAI_LAUNCH(fl_store_kernel, fl_grid(H, W, P), dim3(FL_THREADS), 0, st, state[cur], P, HW0, H, W, flow);
    return viai_launch_status();
}

extern "C" int viai_optical_flow_host(const unsigned char* frames, long frame_stride, int N, int H, int W, int C, int bgr, float tau, float lam,
                                      float theta, int scales, int warps, int iterations, int iters_per_launch, float* flow) {
    if (!fl_args_ok(frames, frame_stride, N, H, W, C, tau, lam, theta, scales, warps, iterations, iters_per_launch, flow))
        return (int)hipErrorInvalidValue;
    const FlLevels L = fl_levels(H, W, scales);
    const long HW0 = (long)H * W;
    const float lt = lam * theta, taut = tau / theta;
    const int ro = bgr ? 2 : 0, bo = bgr ? 0 : 2;
    std::vector<float> pyr((size_t)N * L.total);
    for (int f = 0; f < N; ++f) {
        float* p = pyr.data() + (long)f * L.total;
        for (long i = 0; i < HW0; ++i) {
            const unsigned char* px = frames + (long)f * frame_stride + i * C;
            p[i] = C == 1 ? (float)px[0] : fl_grey(px[ro], px[1], px[bo]);
        }
        for (int l = 1; l < L.S; ++l)
            for (int y = 0; y < L.h[l]; ++y)
                for (int x = 0; x < L.w[l]; ++x) p[L.off[l] + (long)y * L.w[l] + x] = fl_down(p + L.off[l - 1], L.h[l - 1], L.w[l - 1], y, x);
    }
    std::vector<float> u(HW0), v(HW0), t0(HW0), t1(HW0), p11(HW0), p12(HW0), p21(HW0), p22(HW0);
    std::vector<FlWarp> c(HW0);
    for (int z = 0; z < N - 1; ++z) {
        for (int l = L.S - 1; l >= 0; --l) {
            const int h = L.h[l], w = L.w[l];
            const long n = (long)h * w;
            const float* I0 = pyr.data() + (long)z * L.total + L.off[l];
            const float* I1 = pyr.data() + (long)(z + 1) * L.total + L.off[l];
            if (l == L.S - 1) {
                for (long i = 0; i < n; ++i) u[i] = v[i] = 0.f;
            } else {
                for (int y = 0; y < h; ++y)
                    for (int x = 0; x < w; ++x) {
                        t0[(long)y * w + x] = fl_up(u.data(), L.h[l + 1], L.w[l + 1], y, x);
                        t1[(long)y * w + x] = fl_up(v.data(), L.h[l + 1], L.w[l + 1], y, x);
                    }
                u.swap(t0); v.swap(t1);
            }
            for (long i = 0; i < n; ++i) p11[i] = p12[i] = p21[i] = p22[i] = 0.f;
            for (int wp = 0; wp < warps; ++wp) {
                for (int y = 0; y < h; ++y)
                    for (int x = 0; x < w; ++x) c[(long)y * w + x] = fl_warp(I0, I1, h, w, y, x, u[(long)y * w + x], v[(long)y * w + x]);
                for (int it = 0; it < iterations; ++it) {
                    for (int y = 0; y < h; ++y)
                        for (int x = 0; x < w; ++x) {
                            const long i = (long)y * w + x;
                            const float div_u = fl_bdiff(p11[i], x > 0 ? p11[i - 1] : 0.f, x, w) + fl_bdiff(p12[i], y > 0 ? p12[i - w] : 0.f, y, h);
                            const float div_v = fl_bdiff(p21[i], x > 0 ? p21[i - 1] : 0.f, x, w) + fl_bdiff(p22[i], y > 0 ? p22[i - w] : 0.f, y, h);
                            fl_step_u(lt, theta, c[i], div_u, div_v, &u[i], &v[i]);
                        }
                    for (int y = 0; y < h; ++y)
                        for (int x = 0; x < w; ++x) {
                            const long i = (long)y * w + x;
                            const float ux = x < w - 1 ? u[i + 1] - u[i] : 0.f, uy = y < h - 1 ? u[i + w] - u[i] : 0.f;
                            const float vx = x < w - 1 ? v[i + 1] - v[i] : 0.f, vy = y < h - 1 ? v[i + w] - v[i] : 0.f;
                            fl_step_p(taut, ux, uy, &p11[i], &p12[i]);
                            fl_step_p(taut, vx, vy, &p21[i], &p22[i]);
                        }
                }
            }
        }
        for (long i = 0; i < HW0; ++i) { flow[(2L * z) * HW0 + i] = u[i]; flow[(2L * z + 1) * HW0 + i] = v[i]; }
    }
    return 0;
}

extern "C" int viai_flow_encode_u8(const float* flow, int pairs, int H, int W, float bound, int pad_last, unsigned char* flow_x,
                                   unsigned char* flow_y, void* stream) {
    if (!fl_encode_args_ok(flow, pairs, H, W, bound, flow_x, flow_y)) return (int)hipErrorInvalidValue;
    const long HW = (long)H * W;
    VIAI_LAUNCH(fl_encode_kernel, dim3((unsigned)((HW + FL_THREADS - 1) / FL_THREADS), (unsigned)(pairs + (pad_last ? 1 : 0))), dim3(FL_THREADS), 0,
                (hipStream_t)stream, flow, pairs, HW, bound, flow_x, flow_y);
    return viai_launch_status();
}

extern "C" int viai_flow_encode_u8_host(const float* flow, int pairs, int H, int W, float bound, int pad_last, unsigned char* flow_x,
                                        unsigned char* flow_y) {
    if (!fl_encode_args_ok(flow, pairs, H, W, bound, flow_x, flow_y)) return (int)hipErrorInvalidValue;
    const long HW = (long)H * W;
    for (int z = 0; z < pairs + (pad_last ? 1 : 0); ++z) {
        const int src = z < pairs ? z : pairs - 1;
        for (long i = 0; i < HW; ++i) {
            flow_x[(long)z * HW + i] = fl_encode(flow[(2L * src) * HW + i], bound);
            flow_y[(long)z * HW + i] = fl_encode(flow[(2L * src + 1) * HW + i], bound);
        }
    }
    return 0;
}
