// From a 1-bit-per-sample damage mask to ordered (start, length) lists: the pieces gap_detect.hip (which builds the mask from the samples) and
// click_detect.hip (which builds it from a prediction residual) share.  Rule: include/viai_hip.h; layout: DESIGN.md 11.2m.
//
//   device   the per-tile table, the wave scans, the walk over the runs of one mask word (gd_word_sum), what a lane knows about its tile
//            (gd_lane), and gd_tile_summary: the mask row and the launch-1 fields of one tile, written by the wave that holds the tile's 64 words
//   host     viai_gd_launch_runs (gap_detect.hip): launches 2 and 3 over a mask and its summaries; gd_runs_host: the run rule sample by sample
#pragma once
#include "viai_common.h"

namespace {

constexpr int GD_TILE = VIAI_GAP_DETECT_TILE;
constexpr int GD_WORDS = GD_TILE / 64;
constexpr int GD_THREADS = 256;
constexpr int GD_WAVES = GD_THREADS / 64;
constexpr int GD_CHUNK = 256;                                  // samples a wave takes per load: 64 lanes x 4
constexpr int GD_CHUNKS = GD_TILE / (GD_WAVES * GD_CHUNK);     // ... and how many of them
constexpr int GD_NONE = -1;                                    // no position in front (ends and starts are >= 0)
constexpr int GD_FAR = 0x7fffffff;                             // no position behind
static_assert(GD_WORDS == 64, "one mask word of a tile per lane of a wave");
static_assert(GD_CHUNKS * GD_WAVES * GD_CHUNK == GD_TILE, "whole chunks");

// per-tile table in the workspace, field-major: tab[(field * tiles_total) + b * ntiles + t]
enum : int {
    GD_FG,      // launch 1: first good index of the tile, tile-relative; GD_TILE when every sample is damaged
    GD_LG,      //           last good index, tile-relative; -1
    GD_HP,      //           1 when the sample in front of the tile is damaged (a run at the tile's head is then no start)
    GD_NI,      //           kept runs that start and end inside the tile
    GD_FI,      //           start of the first of them (GD_FAR)
    GD_LI,      //           end of the last of them (GD_NONE)
    GD_HI,      //           heads among them, the first one not counted
    GD_LHI,     //           start of the last of those heads (GD_NONE)
    GD_NG,      // launch 2: first good index of the row behind the tile; the row's length when there is none
    GD_PREV,    //           end of the last kept run that starts in front of the tile (GD_NONE)
    GD_HEADS,   //           merged runs that begin in the tile
    GD_OFF,     //           ... and how many begin in front of it
    GD_CUR,     //           start of the last merged run that begins in front of the tile (GD_NONE)
    GD_FIELDS
};

struct OpMin { __device__ int operator()(int a, int b) const { return a < b ? a : b; } };
struct OpMax { __device__ int operator()(int a, int b) const { return a > b ? a : b; } };
struct OpAdd { __device__ int operator()(int a, int b) const { return a + b; } };

template <class Op>
__device__ __forceinline__ int gd_wave_all(int v, Op op) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
    return v;
}
// exclusive scans over the lanes of a wave: lanes in front (prefix) or behind (suffix)
template <class Op>
__device__ __forceinline__ int gd_wave_prefix(int v, int id, Op op, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(v, o, 64);
        if (lane >= o) v = op(u, v);
    }
    const int e = __shfl_up(v, 1, 64);
    return lane == 0 ? id : e;
}
template <class Op>
__device__ __forceinline__ int gd_wave_suffix(int v, int id, Op op, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_down(v, o, 64);
        if (lane + o < 64) v = op(v, u);
    }
    const int e = __shfl_down(v, 1, 64);
    return lane == 63 ? id : e;
}

// The kept runs of one piece (a word, a tile), as far as the piece itself can tell
struct GdSum {
    int nk;     // kept runs
    int f;      // start of the first (GD_FAR)
    int le;     // end of the last (GD_NONE)
    int h;      // heads among them, the first kept run not counted
    int lh;     // start of the last of those heads (GD_NONE)
};

// runs that START in the word m whose first sample is w0.  prev: 1 when the sample in front of the word is damaged.  nz: the first good index
// behind the word, for the run that leaves it; negative when not known yet: such a run is not kept here.
__device__ __forceinline__ GdSum gd_word_sum(unsigned long long m, unsigned long long prev, int w0, int nz, int min_len, int mw) {
    GdSum r = {0, GD_FAR, GD_NONE, 0, GD_NONE};
    unsigned long long starts = m & ~((m << 1) | prev);
    while (starts != 0) {
        const int s = __builtin_ctzll(starts);
        starts &= starts - 1;
        const unsigned long long z = ~m & (~0ull << s);
        const int sa = w0 + s, e = z != 0 ? w0 + __builtin_ctzll(z) : nz;
        if (e - sa < min_len) continue;
        if (r.nk == 0) {
            r.f = sa;
        } else if (sa - r.le > mw) {
            r.h += 1;
            r.lh = sa;
        }
        r.le = e;
        r.nk += 1;
    }
    return r;
}

// what the lanes of one wave know about the tile whose mask word they hold
struct GdLane {
    unsigned long long prev;
    int nz_rel;     // first good index behind the word, tile-relative; GD_FAR: none in the tile
    int fz, lz;     // first / last good index of the word, tile-relative (GD_FAR / -1)
};
__device__ __forceinline__ GdLane gd_lane(unsigned long long m, int hp, int lane) {
    GdLane r;
    const int top = (int)(m >> 63), up = __shfl_up(top, 1, 64);
    r.prev = (unsigned long long)(lane == 0 ? hp : up);
    const unsigned long long g = ~m;
    r.fz = g != 0 ? 64 * lane + __builtin_ctzll(g) : GD_FAR;
    r.lz = g != 0 ? 64 * lane + 63 - __builtin_clzll(g) : -1;
    r.nz_rel = gd_wave_suffix(r.fz, GD_FAR, OpMin(), lane);
    return r;
}

__device__ __forceinline__ int gd_row_len(const int* __restrict__ lengths, int b, int n) {
    int len = lengths != nullptr ? lengths[b] : n;
    len = len < 0 ? 0 : len;
    return len > n ? n : len;
}

// One whole wave, lane = word: tile `at` (first sample `base`) gets its mask row and its launch-1 summary from the runs that end inside the tile.
// m: the lane's mask word; hp: 1 when the sample in front of the tile is damaged.
__device__ __forceinline__ void gd_tile_summary(unsigned long long m, int hp, long at, int base, int lane, int min_len, int mw,
                                                unsigned long long* __restrict__ mask, int* __restrict__ tab, long tiles_total) {
    mask[at * GD_WORDS + lane] = m;
    const GdLane L = gd_lane(m, hp, lane);
    const int nz = L.nz_rel == GD_FAR ? -1 : base + L.nz_rel;               // a run that leaves the tile: not known here, launch 2 adds it
    const GdSum s = gd_word_sum(m, L.prev, base + 64 * lane, nz, min_len, mw);
    const int carry = gd_wave_prefix(s.le, GD_NONE, OpMax(), lane);
    const bool fh = s.nk > 0 && carry != GD_NONE && s.f - carry > mw;       // the tile's first kept run is left open (carry == GD_NONE)
    const int fg = gd_wave_all(L.fz, OpMin()), lg = gd_wave_all(L.lz, OpMax());
    const int ni = gd_wave_all(s.nk, OpAdd()), fi = gd_wave_all(s.f, OpMin()), li = gd_wave_all(s.le, OpMax());
    const int hi = gd_wave_all(s.h + (fh ? 1 : 0), OpAdd());
    const int lhi = gd_wave_all(s.lh != GD_NONE ? s.lh : (fh ? s.f : GD_NONE), OpMax());
    if (lane < 8) {
        const int val = lane == GD_FG ? (fg == GD_FAR ? GD_TILE : fg)
                      : lane == GD_LG ? lg
                      : lane == GD_HP ? hp
                      : lane == GD_NI ? ni
                      : lane == GD_FI ? fi
                      : lane == GD_LI ? li
                      : lane == GD_HI ? hi : lhi;
        tab[(long)lane * tiles_total + at] = val;
    }
}

inline long gd_tiles(long n) { return (n + GD_TILE - 1) / GD_TILE; }

inline bool gd_shape_ok(int B, long n, int K) {
    return B >= 1 && n >= 1 && K >= 1 && n < (1L << 31) && (long)B * gd_tiles(n) <= 0x7fffffffL;
}

// steps 2 to 4 of the rule over one row, sample by sample: damaged(i) for i in [0, len) -> the row's K entries and its true count
template <class Damaged>
inline int gd_runs_host(long len, Damaged damaged, int min_len, int merge_within, int K, int* st, int* ln) {
    long cnt = 0, cs = 0, ce = 0;
    bool open = false;
    auto close = [&]() {
        if (cnt < K) {
            st[cnt] = (int)cs;
            ln[cnt] = (int)(ce - cs);
        }
        ++cnt;
    };
    long i = 0;
    while (i < len) {
        if (!damaged(i)) {
            ++i;
            continue;
        }
        const long s = i;
        while (i < len && damaged(i)) ++i;
        if (i - s < min_len) continue;
        if (open && s - ce <= merge_within) {
            ce = i;
            continue;
        }
        if (open) close();
        cs = s;
        ce = i;
        open = true;
    }
    if (open) close();
    for (long k = cnt < K ? cnt : K; k < K; ++k) st[k] = ln[k] = 0;
    return (int)cnt;
}

}  // namespace

// gap_detect.hip: launches 2 and 3 (gd_rows_kernel, gd_emit_kernel) over a mask and the launch-1 fields of its table; the launch status
int viai_gd_launch_runs(const int* lengths, int n, int ntiles, int min_len, int merge_within, int K, const unsigned long long* mask, int* tab,
                        long tiles_total, int* count, int* start, int* length, hipStream_t st);
