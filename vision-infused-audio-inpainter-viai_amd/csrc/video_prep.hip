// Video front end (gfx950): motion bounding box from the flow stacks, then crop + square pad + resize + flip + crop + normalise of the frames.
// Contract and rule: include/viai_hip.h; launches, bytes moved and measured rates: DESIGN.md 11.2n.
//
//   vp_motion_kernel   one wave per tile of 4 rows x 256 pixels.  A lane owns 16 adjacent pixels of one row, loads them from both stacks with one
//                      16-byte load each per frame (byte loads where the 16 pixels are not 16-byte aligned or cross the row's end; the missing
//                      pixels read as 127 and sum to 0), and keeps the 16 int32 sums in registers over the frames.  |fx - 127| + |fy - 127| of
//                      one pixel is one v_perm_b32 (the two bytes side by side, zeros above) and one v_sad_u8 against 0x00007f7f.  At the end
//                      the tile's column flags (OR over its 4 rows) and row flags (a ballot) go out as plain byte stores.
//   vp_box_kernel      one block.  Per axis: OR the tiles' flags into an occupancy byte per index in LDS, then four block-wide min / max
//                      reductions give the closed form of find_cluster.  Writes the five ints.
//   vp_table_kernel    one block.  Reads the box from device memory, clamps it to the frame, resolves the crop and the pad, and makes the R-entry
//                      coefficient table once.  The header and the table live in the caller's workspace.
//   vp_resize_kernel   one lane per pixel of the R x R image, uint8 out (inspection and the equality test)
//   vp_prepare_kernel  one lane per pixel of the size x size window, fp32 NHWC4 (one 16-byte store) or planar out
#include <cmath>
#include <cstdlib>
#include <vector>

#include "viai_common.h"
#include "viai_internal.h"

namespace {

constexpr int VP_TW = VIAI_MOTION_TILE_W;
constexpr int VP_TH = VIAI_MOTION_TILE_H;
constexpr int VP_PX = 16;                        // pixels of a lane
constexpr int VP_MAX_DIM = 1 << 15;              // H, W below this
constexpr int VP_MAX_N = 1 << 22;                // 2^22 frames x 256 per pixel and frame stays inside int32
constexpr int VP_MAX_R = 1 << 13;
constexpr int VP_HEAD = 8;                       // ints in front of the table: x0, y0, cw, ch, side, padx, pady, 0
constexpr int VP_BOX_THREADS = 1024;
static_assert(VP_TW == 16 * VP_PX && VP_TH * 16 == 64, "a tile is one wave: 4 rows of 16 lanes of 16 pixels");

inline int vp_tiles_x(int W) { return (W + VP_TW - 1) / VP_TW; }
inline int vp_tiles_y(int H) { return (H + VP_TH - 1) / VP_TH; }
inline bool vp_dim_ok(int H, int W) { return H >= 1 && W >= 1 && H < VP_MAX_DIM && W < VP_MAX_DIM; }

// ------------------------------------------------------------------------------------------------ the rule's shared pieces (host and device)
struct VpGeo { int x0, y0, cw, ch, side, padx, pady; };

__host__ __device__ inline int vp_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the crop of a box inside an H x W frame, and where it sits in its padded square
__host__ __device__ inline VpGeo vp_geo(const int* box, int H, int W) {
    int w0 = vp_clamp(box[0], 0, W), w1 = vp_clamp(box[1], w0, W), h0 = vp_clamp(box[2], 0, H), h1 = vp_clamp(box[3], h0, H);
    if (box[4] == 0 || w1 - w0 < 1 || h1 - h0 < 1) { w0 = 0; w1 = W; h0 = 0; h1 = H; }
    VpGeo g;
    g.x0 = w0; g.y0 = h0; g.cw = w1 - w0; g.ch = h1 - h0;
    g.side = g.ch > g.cw ? g.ch : g.cw;
    g.padx = (g.side - g.cw) / 2;
    g.pady = (g.side - g.ch) / 2;
    return g;
}

// table entry d of side -> R: first tap s and the coefficients (c0, c1) of taps s and min(s + 1, side - 1)
__host__ __device__ inline void vp_coef(int d, int side, int R, int* s, int* c0, int* c1) {
#pragma clang fp contract(off)
    const double scale = (double)side / (double)R;
    const double prod = ((double)d + 0.5) * scale;
    const float f = (float)(prod - 0.5);
    const float fl = floorf(f);
    int si = (int)fl;
    float a = f - fl;
    if (si < 0) { si = 0; a = 0.f; }
    if (si >= side - 1) { si = side - 1; a = 0.f; }
    const float one_minus = 1.f - a;
    *s = si;
    *c0 = (int)rintf(one_minus * 2048.f);
    *c1 = (int)rintf(a * 2048.f);
}

__host__ __device__ inline int vp_vertical(int b0, int b1, int h0, int h1) {
    const int q = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2;
    return q > 255 ? 255 : q;
}

// channel planes of the source: pixel (f, y, x) of channel c is ch[c][f * fstride + (y * W + x) * ps]
struct VpSrc {
    const unsigned char* ch[4];
    long fstride;
    int ps, N, H, W, C;
};

inline VpSrc vp_src(const unsigned char* src0, const unsigned char* src1, long fstride, int N, int H, int W, int C, int bgr) {
    VpSrc s;
    for (int c = 0; c < 4; ++c) s.ch[c] = src0;
    if (src1 != nullptr) {
        s.ch[0] = bgr ? src1 : src0;
        s.ch[1] = bgr ? src0 : src1;
        s.ps = 1;
    } else {
        for (int c = 0; c < C; ++c) s.ch[c] = src0 + (bgr ? C - 1 - c : c);
        s.ps = C;
    }
    s.fstride = fstride; s.N = N; s.H = H; s.W = W; s.C = C;
    return s;
}

// pixel (sy, sx) of the padded square of frame plane `base`
__host__ __device__ inline int vp_px(const unsigned char* base, const VpGeo& g, int W, int ps, int sy, int sx) {
    const int yy = sy - g.pady, xx = sx - g.padx;
    if ((unsigned)yy >= (unsigned)g.ch || (unsigned)xx >= (unsigned)g.cw) return 127;
    return base[((long)(g.y0 + yy) * W + (g.x0 + xx)) * ps];
}

// output pixel (ry, rx) of the R x R image, channel plane `base` of one frame; (s, c0 | c1 << 16) per table entry
__host__ __device__ inline int vp_sample(const unsigned char* base, const VpGeo& g, int W, int ps, int sy0, int b, int sx0, int a) {
    const int sy1 = sy0 + 1 < g.side ? sy0 + 1 : g.side - 1, sx1 = sx0 + 1 < g.side ? sx0 + 1 : g.side - 1;
    const int a0 = a & 0xffff, a1 = a >> 16, b0 = b & 0xffff, b1 = b >> 16;
    const int h0 = vp_px(base, g, W, ps, sy0, sx0) * a0 + vp_px(base, g, W, ps, sy0, sx1) * a1;
    const int h1 = vp_px(base, g, W, ps, sy1, sx0) * a0 + vp_px(base, g, W, ps, sy1, sx1) * a1;
    return vp_vertical(b0, b1, h0, h1);
}

// find_cluster from the four extremes of an axis: first / last occupied index, first occupied v with v + 5 occupied (or -1), last occupied
// v with v - 5 occupied (or -1).  last < 0: nothing occupied.
__host__ __device__ inline void vp_cluster(int first, int last, int first_p5, int last_m5, int* mn, int* mx) {
    if (last < 0) { *mn = *mx = 0; return; }
    int lo = first_p5 >= 0 ? first_p5 : last, hi = last_m5 >= 0 ? last_m5 : first;
    if (lo > hi) hi = lo;
    *mn = lo; *mx = hi;
}

// ------------------------------------------------------------------------------------------------ motion pass
__global__ __launch_bounds__(64) void vp_motion_kernel(const unsigned char* __restrict__ fx, const unsigned char* __restrict__ fy, long fstride,
                                                       int N, int H, int W, unsigned char* __restrict__ colflag,
                                                       unsigned char* __restrict__ rowflag) {
    const int lane = threadIdx.x, tx = blockIdx.x, ty = blockIdx.y;
    const int x = tx * VP_TW + (lane & 15) * VP_PX, y = ty * VP_TH + (lane >> 4);
    const int cnt = (y < H && x < W) ? (W - x < VP_PX ? W - x : VP_PX) : 0;          // pixels of this lane that exist
    const long off = cnt > 0 ? (long)y * W + x : 0;
    const bool vec = cnt == VP_PX &&
                     (((reinterpret_cast<uintptr_t>(fx) + (uintptr_t)off) | (reinterpret_cast<uintptr_t>(fy) + (uintptr_t)off) | (uintptr_t)fstride) & 15) == 0;
    int acc[VP_PX];
#pragma unroll
    for (int i = 0; i < VP_PX; ++i) acc[i] = 0;
    const unsigned char* px = fx + off;
    const unsigned char* py = fy + off;
#pragma unroll 4
    for (int n = 0; n < N; ++n, px += fstride, py += fstride) {
        u32x4 a = {0x7f7f7f7fu, 0x7f7f7f7fu, 0x7f7f7f7fu, 0x7f7f7f7fu}, b = a;
        if (vec) {
            a = *reinterpret_cast<const u32x4*>(px);
            b = *reinterpret_cast<const u32x4*>(py);
        } else {
#pragma unroll
            for (int i = 0; i < VP_PX; ++i) {
                if (i < cnt) {
                    const unsigned sh = 8u * (i & 3), keep = ~(0xffu << sh);
                    a[i >> 2] = (a[i >> 2] & keep) | ((unsigned)px[i] << sh);
                    b[i >> 2] = (b[i >> 2] & keep) | ((unsigned)py[i] << sh);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                // byte 0 = byte k of a[j], byte 1 = byte k of b[j], bytes 2 and 3 = 0 (selector 0x0c)
                const unsigned both = __builtin_amdgcn_perm(a[j], b[j], 0x0c0c0000u | ((unsigned)k << 8) | (unsigned)(4 + k));
                acc[4 * j + k] = (int)__builtin_amdgcn_sad_u8(both, 0x00007f7fu, (unsigned)acc[4 * j + k]);
            }
        }
    }
    unsigned own = 0;
#pragma unroll
    for (int i = 0; i < VP_PX; ++i) own |= (acc[i] > 2 * N ? 1u : 0u) << i;
    // rows: lanes 16 r .. 16 r + 15 hold row r of the tile
    const unsigned long long any = __ballot(own != 0);
    if (lane < VP_TH && ty * VP_TH + lane < H)
        rowflag[(long)tx * H + ty * VP_TH + lane] = ((any >> (16 * lane)) & 0xffffull) != 0 ? 1 : 0;
    // columns: OR over the 4 rows; the lanes of row 0 write (row 0 of a tile always exists, so their cnt is the tile's)
    unsigned col = own;
    col |= (unsigned)__shfl_xor((int)col, 16, 64);
    col |= (unsigned)__shfl_xor((int)col, 32, 64);
    if (lane < 16) {
        unsigned char* c = colflag + (long)ty * W + x;
#pragma unroll
        for (int i = 0; i < VP_PX; ++i)
            if (i < cnt) c[i] = (unsigned char)((col >> i) & 1u);
    }
}

// max over the block of four ints at once; every thread calls it, every thread gets the result
__device__ __forceinline__ void vp_block_max4(int (&v)[4], int (*red)[4]) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int k = 0; k < 4; ++k) { const int t = __shfl_xor(v[k], o, 64); v[k] = t > v[k] ? t : v[k]; }
    }
    __syncthreads();                                     // the last use of red is over
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < 4; ++k) red[threadIdx.x >> 6][k] = v[k];
    __syncthreads();
    for (int w = 0; w < VP_BOX_THREADS / 64; ++w)
        for (int k = 0; k < 4; ++k) v[k] = red[w][k] > v[k] ? red[w][k] : v[k];
}

// flags: [T][L] bytes.  occ: L bytes of LDS.  Returns min and max of find_cluster on the axis to every thread.
__device__ __forceinline__ void vp_axis(const unsigned char* __restrict__ flags, int T, int L, unsigned char* occ, int (*red)[4], int* mn, int* mx) {
    __syncthreads();                                     // occ may still be read for the axis before
    for (int v = threadIdx.x; v < L; v += VP_BOX_THREADS) {
        unsigned o = 0;
        for (int t = 0; t < T; ++t) o |= flags[(long)t * L + v];
        occ[v] = o != 0 ? 1 : 0;
    }
    __syncthreads();
    const int none = -0x7fffffff;
    int e[4] = {none, -1, none, -1};                     // -first, last, -first_p5, last_m5
    for (int v = threadIdx.x; v < L; v += VP_BOX_THREADS) {
        if (!occ[v]) continue;
        e[0] = -v > e[0] ? -v : e[0];
        e[1] = v > e[1] ? v : e[1];
        if (v + 5 < L && occ[v + 5]) e[2] = -v > e[2] ? -v : e[2];
        if (v >= 5 && occ[v - 5]) e[3] = v > e[3] ? v : e[3];
    }
    vp_block_max4(e, red);
    vp_cluster(-e[0], e[1], e[2] == none ? -1 : -e[2], e[3], mn, mx);
}

__global__ __launch_bounds__(VP_BOX_THREADS) void vp_box_kernel(const unsigned char* __restrict__ colflag, const unsigned char* __restrict__ rowflag,
                                                                int H, int W, int tiles_x, int tiles_y, int min_extent, int* __restrict__ box) {
    __shared__ unsigned char occ[VP_MAX_DIM];
    __shared__ int red[VP_BOX_THREADS / 64][4];
    int w0, w1, h0, h1;
    vp_axis(colflag, tiles_y, W, occ, red, &w0, &w1);
    vp_axis(rowflag, tiles_x, H, occ, red, &h0, &h1);
    if (threadIdx.x == 0) {
        box[0] = w0; box[1] = w1; box[2] = h0; box[3] = h1;
        box[4] = (w1 - w0 >= min_extent && h1 - h0 >= min_extent) ? 1 : 0;
    }
}

// ------------------------------------------------------------------------------------------------ table, resize, prepare
__global__ __launch_bounds__(256) void vp_table_kernel(const int* __restrict__ box, int H, int W, int R, int* __restrict__ ws) {
    const VpGeo g = vp_geo(box, H, W);                   // every thread: five uniform loads, no barrier
    if (threadIdx.x == 0) {
        ws[0] = g.x0; ws[1] = g.y0; ws[2] = g.cw; ws[3] = g.ch; ws[4] = g.side; ws[5] = g.padx; ws[6] = g.pady; ws[7] = 0;
    }
    for (int d = threadIdx.x; d < R; d += 256) {
        int s, c0, c1;
        vp_coef(d, g.side, R, &s, &c0, &c1);
        ws[VP_HEAD + 2 * d] = s;
        ws[VP_HEAD + 2 * d + 1] = c0 | (c1 << 16);
    }
}

__device__ __forceinline__ VpGeo vp_geo_of(const int* __restrict__ ws) {
    VpGeo g;
    g.x0 = ws[0]; g.y0 = ws[1]; g.cw = ws[2]; g.ch = ws[3]; g.side = ws[4]; g.padx = ws[5]; g.pady = ws[6];
    return g;
}

__device__ __forceinline__ long vp_frame(const VpSrc& s, const int* __restrict__ frames_index, long f) {
    int idx = frames_index != nullptr ? frames_index[f] : (int)f;
    idx = idx < 0 ? 0 : (idx > s.N - 1 ? s.N - 1 : idx);
    return (long)idx * s.fstride;
}

__global__ __launch_bounds__(256) void vp_resize_kernel(VpSrc s, const int* __restrict__ ws, const int* __restrict__ frames_index, long n, int R,
                                                        unsigned char* __restrict__ out) {
    const VpGeo g = vp_geo_of(ws);
    const int2* tab = reinterpret_cast<const int2*>(ws + VP_HEAD);
    const long total = n * R * R;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256L) {
        const int x = (int)(i % R); const long r = i / R; const int y = (int)(r % R); const long f = r / R;
        const long fo = vp_frame(s, frames_index, f);
        const int2 ty = tab[y], tx = tab[x];
        for (int c = 0; c < s.C; ++c) out[i * s.C + c] = (unsigned char)vp_sample(s.ch[c] + fo, g, s.W, s.ps, ty.x, ty.y, tx.x, tx.y);
    }
}

__global__ __launch_bounds__(256) void vp_prepare_kernel(VpSrc s, const int* __restrict__ ws, const int* __restrict__ frames_index, long n, int R,
                                                         int size, int crop_x, int crop_y, int flip, int nchw, float* __restrict__ out) {
    const VpGeo g = vp_geo_of(ws);
    const int2* tab = reinterpret_cast<const int2*>(ws + VP_HEAD);
    const long total = n * size * size;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256L) {
        const int x = (int)(i % size); const long r = i / size; const int y = (int)(r % size); const long f = r / size;
        const int ry = crop_x + y;
        int rx = crop_y + x;
        if (flip) rx = R - 1 - rx;
        const long fo = vp_frame(s, frames_index, f);
        const int2 ty = tab[ry], tx = tab[rx];
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (c < s.C) v[c] = ((float)vp_sample(s.ch[c] + fo, g, s.W, s.ps, ty.x, ty.y, tx.x, tx.y) - 127.f) / 128.f;
        if (nchw) {
            const long plane = (long)size * size, o = f * s.C * plane + (long)y * size + x;
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (c < s.C) out[o + c * plane] = v[c];
        } else {
            reinterpret_cast<f32x4*>(out)[i] = v;
        }
    }
}

bool vp_motion_args_ok(const void* fx, const void* fy, long fstride, int N, int H, int W, int min_extent, const void* box) {
    return fx != nullptr && fy != nullptr && box != nullptr && N >= 1 && N <= VP_MAX_N && vp_dim_ok(H, W) && fstride >= (long)H * W && min_extent >= 0;
}

bool vp_resize_args_ok(const void* src0, const void* src1, long fstride, int N, int H, int W, int C, const void* box, const int* frames_index,
                       int n, int R, const void* out) {
    if (src0 == nullptr || box == nullptr || out == nullptr || C < 1 || C > 4 || (src1 != nullptr && C != 2)) return false;
    if (N < 1 || N > VP_MAX_N || n < 1 || n > VP_MAX_N || (frames_index == nullptr && n > N) || !vp_dim_ok(H, W) || R < 1 || R > VP_MAX_R) return false;
    return fstride >= (long)H * W * (src1 != nullptr ? 1 : C);
}

}  // namespace

extern "C" long viai_motion_box_ws_bytes(int H, int W) {
    if (!vp_dim_ok(H, W)) return 0;
    return (long)vp_tiles_y(H) * W + (long)vp_tiles_x(W) * H;
}

extern "C" int viai_motion_flags(const unsigned char* flow_x, const unsigned char* flow_y, long frame_stride, int N, int H, int W, void* ws,
                                 void* stream) {
    int dummy = 0;
    if (!vp_motion_args_ok(flow_x, flow_y, frame_stride, N, H, W, 0, &dummy) || ws == nullptr) return (int)hipErrorInvalidValue;
    unsigned char* colflag = static_cast<unsigned char*>(ws);
    VIAI_LAUNCH(vp_motion_kernel, dim3((unsigned)vp_tiles_x(W), (unsigned)vp_tiles_y(H)), dim3(64), 0, (hipStream_t)stream, flow_x, flow_y,
                frame_stride, N, H, W, colflag, colflag + (long)vp_tiles_y(H) * W);
    return viai_launch_status();
}

extern "C" int viai_motion_box_of_flags(const void* ws, int H, int W, int min_extent, int* box, void* stream) {
    if (ws == nullptr || box == nullptr || !vp_dim_ok(H, W) || min_extent < 0) return (int)hipErrorInvalidValue;
    const unsigned char* colflag = static_cast<const unsigned char*>(ws);
    VIAI_LAUNCH(vp_box_kernel, dim3(1), dim3(VP_BOX_THREADS), 0, (hipStream_t)stream, colflag, colflag + (long)vp_tiles_y(H) * W, H, W,
                vp_tiles_x(W), vp_tiles_y(H), min_extent, box);
    return viai_launch_status();
}

extern "C" int viai_motion_box(const unsigned char* flow_x, const unsigned char* flow_y, long frame_stride, int N, int H, int W, int min_extent,
                               int* box, void* ws, void* stream) {
    if (!vp_motion_args_ok(flow_x, flow_y, frame_stride, N, H, W, min_extent, box) || ws == nullptr) return (int)hipErrorInvalidValue;
    const int e = viai_motion_flags(flow_x, flow_y, frame_stride, N, H, W, ws, stream);
    return e != 0 ? e : viai_motion_box_of_flags(ws, H, W, min_extent, box, stream);
}

// Rules 1 - 5 pixel by pixel; find_cluster as the reference walks it.
extern "C" int viai_motion_box_host(const unsigned char* flow_x, const unsigned char* flow_y, long frame_stride, int N, int H, int W,
                                    int min_extent, int* box) {
    if (!vp_motion_args_ok(flow_x, flow_y, frame_stride, N, H, W, min_extent, box)) return (int)hipErrorInvalidValue;
    std::vector<char> occ_w(W, 0), occ_h(H, 0);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            long S = 0;
            for (int n = 0; n < N; ++n) {
                const long at = (long)n * frame_stride + (long)y * W + x;
                S += std::abs((int)flow_x[at] - 127) + std::abs((int)flow_y[at] - 127);
            }
            if (S > 2L * N) occ_w[x] = occ_h[y] = 1;
        }
    auto cluster = [](const std::vector<char>& occ, int* mn, int* mx) {
        std::vector<int> o;
        for (int v = 0; v < (int)occ.size(); ++v)
            if (occ[v]) o.push_back(v);
        if (o.empty()) { *mn = *mx = 0; return; }
        auto has = [&](int v) { return v >= 0 && v < (int)occ.size() && occ[v] != 0; };
        const int len = (int)o.size();
        int lo = 0, hi = len - 1;
        for (int k = 0; k < len - 1; ++k)
            if (!has(o[lo] + 5)) ++lo;
        for (int k = 0; k < len - 1; ++k)
            if (!has(o[hi] - 5)) --hi;
        *mn = o[lo];
        *mx = o[hi] < o[lo] ? o[lo] : o[hi];
    };
    cluster(occ_w, &box[0], &box[1]);
    cluster(occ_h, &box[2], &box[3]);
    box[4] = (box[1] - box[0] >= min_extent && box[3] - box[2] >= min_extent) ? 1 : 0;
    return 0;
}

extern "C" long viai_video_prep_ws_bytes(int R) {
    if (R < 1 || R > VP_MAX_R) return 0;
    return (long)(VP_HEAD + 2 * R) * (long)sizeof(int);
}

extern "C" int viai_video_resize_u8(const unsigned char* src0, const unsigned char* src1, long frame_stride, int N, int H, int W, int C, int bgr,
                                    const int* box, const int* frames_index, int n, int R, unsigned char* out, void* ws, void* stream) {
    if (!vp_resize_args_ok(src0, src1, frame_stride, N, H, W, C, box, frames_index, n, R, out) || ws == nullptr ||
        (reinterpret_cast<uintptr_t>(ws) & 7) != 0)
        return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    const VpSrc s = vp_src(src0, src1, frame_stride, N, H, W, C, bgr);
    VIAI_LAUNCH(vp_table_kernel, dim3(1), dim3(256), 0, st, box, H, W, R, static_cast<int*>(ws));
    VIAI_LAUNCH(vp_resize_kernel, dim3(viai_ew_blocks((long)n * R * R)), dim3(256), 0, st, s, static_cast<const int*>(ws), frames_index, (long)n, R, out);
    return viai_launch_status();
}

extern "C" int viai_video_prepare(const unsigned char* src0, const unsigned char* src1, long frame_stride, int N, int H, int W, int C, int bgr,
                                  const int* box, const int* frames_index, int n, int R, int size, int crop_x, int crop_y, int flip, int nchw,
                                  float* out, void* ws, void* stream) {
    if (!vp_resize_args_ok(src0, src1, frame_stride, N, H, W, C, box, frames_index, n, R, out) || ws == nullptr ||
        (reinterpret_cast<uintptr_t>(ws) & 7) != 0 || (reinterpret_cast<uintptr_t>(out) & 15) != 0)
        return (int)hipErrorInvalidValue;
    if (size < 1 || size > R || crop_x < 0 || crop_y < 0 || crop_x > R - size || crop_y > R - size) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    const VpSrc s = vp_src(src0, src1, frame_stride, N, H, W, C, bgr);
    VIAI_LAUNCH(vp_table_kernel, dim3(1), dim3(256), 0, st, box, H, W, R, static_cast<int*>(ws));
    VIAI_LAUNCH(vp_prepare_kernel, dim3(viai_ew_blocks((long)n * size * size)), dim3(256), 0, st, s, static_cast<const int*>(ws), frames_index, (long)n, R,
                size, crop_x, crop_y, flip, nchw, out);
    return viai_launch_status();
}

extern "C" int viai_video_resize_u8_host(const unsigned char* src0, const unsigned char* src1, long frame_stride, int N, int H, int W, int C,
                                         int bgr, const int* box, const int* frames_index, int n, int R, unsigned char* out) {
    if (!vp_resize_args_ok(src0, src1, frame_stride, N, H, W, C, box, frames_index, n, R, out)) return (int)hipErrorInvalidValue;
    const VpSrc s = vp_src(src0, src1, frame_stride, N, H, W, C, bgr);
    const VpGeo g = vp_geo(box, H, W);
    std::vector<int> ts(R), tc(R);
    for (int d = 0; d < R; ++d) {
        int c0, c1;
        vp_coef(d, g.side, R, &ts[d], &c0, &c1);
        tc[d] = c0 | (c1 << 16);
    }
    for (int f = 0; f < n; ++f) {
        const int idx = vp_clamp(frames_index != nullptr ? frames_index[f] : f, 0, N - 1);
        for (int y = 0; y < R; ++y)
            for (int x = 0; x < R; ++x)
                for (int c = 0; c < C; ++c)
                    out[(((long)f * R + y) * R + x) * C + c] =
                        (unsigned char)vp_sample(s.ch[c] + (long)idx * frame_stride, g, W, s.ps, ts[y], tc[y], ts[x], tc[x]);
    }
    return 0;
}
