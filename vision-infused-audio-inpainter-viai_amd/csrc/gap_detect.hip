// Where a waveform is damaged (gfx950): runs of non-finite, silent or clipped samples of every row of a batch, as ordered (start, length) lists.
// Contract and rule: include/viai_hip.h; layout, bound and measured rate: DESIGN.md 11.2m.
//
// Three launches for the batch, no atomics, nothing allocated, nothing synced:
//   1  gd_mask_kernel    one block per TILE of 4096 samples.  Reads the samples once (16-byte loads where the row is 16-byte aligned), writes the
//                        1-bit-per-sample damage mask (64 words of 64 bits, each word a wave64 ballot) and the tile's SUMMARY: everything about the
//                        runs that start AND end inside the tile, plus where its first and last good samples are.
//   2  gd_rows_kernel    one block per ROW over the summaries.  A suffix scan gives every tile the first good index behind it (the end of a run
//                        that leaves the tile), a prefix scan the end of the last kept run in front of it; with both every tile's number of
//                        merged runs is known, and an exclusive sum of those is where the tile's runs go.  Writes count, the last run's length
//                        and the zero padding.
//   3  gd_emit_kernel    one wave per tile that holds a run to write.  Walks the tile's mask again, now with the carries of launch 2, and
//                        writes start[k], and length[k - 1] when run k begins (the run before it is then complete).
//
// A run belongs to the word, and the tile, it STARTS in.  Inside a word (one lane) the runs are walked bit by bit with ctz; a run that leaves its
// word ends at the next good index of the words behind (suffix minimum over the lanes), one that leaves the tile at the tile's `ng` (launch 2).
// Kept runs merge when the distance to the kept run before them is <= merge_within, so the output index of a run is the number of kept runs in
// front of it that did NOT merge ("heads").  Words combine into tiles and tiles into rows by the same rule (GdSum): the heads of a piece are
// known up to its first kept run, which needs the end of the last kept run in front of the piece.
#include <cmath>
#include <cstring>

#include "viai_common.h"
#include "viai_internal.h"
#include "viai_gap_runs.h"                                      // the table, the wave scans, the word walk and the tile summary: shared with click_detect.hip

namespace {

// exclusive scan over the threads of a block in the order `pos` (a permutation of 0 .. GD_THREADS - 1); *total: the reduction of all
template <class Op>
__device__ int gd_block_scan(int v, int id, Op op, int* sh, int pos, int* total) {
    sh[pos] = v;
    __syncthreads();
    for (int o = 1; o < GD_THREADS; o <<= 1) {
        const int mine = sh[pos], u = pos >= o ? sh[pos - o] : id;
        __syncthreads();
        sh[pos] = op(u, mine);
        __syncthreads();
    }
    const int ex = pos > 0 ? sh[pos - 1] : id;
    *total = sh[GD_THREADS - 1];
    __syncthreads();
    return ex;
}

// the rule on the bits: |x| as an unsigned integer orders like |x| for every non-NaN value, a NaN lies above the infinity.  Damaged unless
// thr < |x| < hi, hi = clip > 0 ? clip : inf: not finite, |x| <= thr, |x| >= clip.  Independent of the denormal mode.
__device__ __forceinline__ bool gd_damaged(float x, unsigned thr_bits, unsigned hi_bits) {
    const unsigned a = __float_as_uint(x) & 0x7fffffffu;
    return !(a > thr_bits && a < hi_bits);
}

// the same walk with the carries known: prev_end, the end of the last kept run in front of the word (GD_NONE); head_start, the start of the
// merged run that is open there; idx, the merged runs that begin in front.  Run k writes start[k], and length[k - 1] of the run it closes.
__device__ __forceinline__ void gd_word_emit(unsigned long long m, unsigned long long prev, int w0, int nz, int min_len, int mw, int prev_end,
                                             int head_start, int idx, int K, int* __restrict__ start, int* __restrict__ length) {
    unsigned long long starts = m & ~((m << 1) | prev);
    while (starts != 0 && idx <= K) {
        const int s = __builtin_ctzll(starts);
        starts &= starts - 1;
        const unsigned long long z = ~m & (~0ull << s);
        const int sa = w0 + s, e = z != 0 ? w0 + __builtin_ctzll(z) : nz;
        if (e - sa < min_len) continue;
        if (prev_end == GD_NONE || sa - prev_end > mw) {
            if (idx >= 1) length[idx - 1] = prev_end - head_start;          // idx <= K here
            if (idx < K) start[idx] = sa;
            head_start = sa;
            idx += 1;
        }
        prev_end = e;
    }
}

__global__ __launch_bounds__(GD_THREADS) void gd_mask_kernel(const float* __restrict__ wav, const int* __restrict__ lengths, long stride, int n,
                                                             int ntiles, unsigned thr_bits, unsigned hi_bits, int min_len, int mw,
                                                             unsigned long long* __restrict__ mask, int* __restrict__ tab, long tiles_total) {
    __shared__ unsigned long long sm[GD_WORDS];
    const int b = blockIdx.x / ntiles, t = blockIdx.x - b * ntiles;
    const int len = gd_row_len(lengths, b, n);
    const int base = t * GD_TILE;                                           // < 2^31: ntiles GD_TILE <= 2^31 (checked by the host)
    const float* __restrict__ xr = wav + (long)b * stride;
    const bool vec = (reinterpret_cast<uintptr_t>(xr) & 15) == 0;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    f32x4 v[GD_CHUNKS];
    // samples at and beyond len are never read: they do not exist (and beyond n they are not the row's memory)
#pragma unroll
    for (int c = 0; c < GD_CHUNKS; ++c) {
        const int i = base + (c * GD_WAVES + wv) * GD_CHUNK + 4 * lane;    // <= 2^31 - 4
        if (vec && i <= len - 4) {
            v[c] = *reinterpret_cast<const f32x4*>(xr + i);
        } else {
            v[c].x = i < len ? xr[i] : 0.f;
            v[c].y = i + 1 < len ? xr[i + 1] : 0.f;
            v[c].z = i + 2 < len ? xr[i + 2] : 0.f;
            v[c].w = i + 3 < len ? xr[i + 3] : 0.f;
        }
    }
#pragma unroll
    for (int c = 0; c < GD_CHUNKS; ++c) {
        const int q = c * GD_WAVES + wv, i = base + q * GD_CHUNK + 4 * lane;
        // lane l holds samples 4 l .. 4 l + 3 of the chunk: four ballots, bit l of ballot k = sample 4 l + k
        const unsigned long long m0 = __ballot(i < len && gd_damaged(v[c].x, thr_bits, hi_bits));
        const unsigned long long m1 = __ballot(i + 1 < len && gd_damaged(v[c].y, thr_bits, hi_bits));
        const unsigned long long m2 = __ballot(i + 2 < len && gd_damaged(v[c].z, thr_bits, hi_bits));
        const unsigned long long m3 = __ballot(i + 3 < len && gd_damaged(v[c].w, thr_bits, hi_bits));
        // ... and into sample order: sample 64 w + l of the chunk sits in ballot l % 4 at bit 16 w + l / 4, so lane l picks its ballot once
        // and a second ballot per word puts bit l of word w in place
        const int k = lane & 3, sh = lane >> 2;
        const unsigned long long sel = k == 0 ? m0 : (k == 1 ? m1 : (k == 2 ? m2 : m3));
        const unsigned long long w0 = __ballot((sel >> sh) & 1ull), w1 = __ballot((sel >> (16 + sh)) & 1ull);
        const unsigned long long w2 = __ballot((sel >> (32 + sh)) & 1ull), w3 = __ballot((sel >> (48 + sh)) & 1ull);
        if (lane == 0) {
            sm[4 * q] = w0;
            sm[4 * q + 1] = w1;
            sm[4 * q + 2] = w2;
            sm[4 * q + 3] = w3;
        }
    }
    __syncthreads();
    if (wv != 0) return;
    // wave 0: lane = word.  The mask goes out as one 512-byte row; the summary from the runs that end inside the tile.
    const long at = (long)b * ntiles + t;
    const int hp = (t > 0 && base - 1 < len && gd_damaged(xr[base - 1], thr_bits, hi_bits)) ? 1 : 0;
    gd_tile_summary(sm[lane], hp, at, base, lane, min_len, mw, mask, tab, tiles_total);
}

// a tile's kept runs once the end of the run that leaves it (ng) is known: the inner ones, then the tail
__device__ __forceinline__ GdSum gd_tile_sum(const int* __restrict__ tab, long tiles_total, long at, int base, int ng, int min_len, int mw) {
    const int lg = tab[GD_LG * tiles_total + at], hp = tab[GD_HP * tiles_total + at];
    const int ni = tab[GD_NI * tiles_total + at], fi = tab[GD_FI * tiles_total + at], li = tab[GD_LI * tiles_total + at];
    const int hi = tab[GD_HI * tiles_total + at], lhi = tab[GD_LHI * tiles_total + at];
    // the tile's last sample is damaged, and its run starts here: behind the last good sample, or at the head of an all-damaged tile
    const bool has_tail = lg != GD_TILE - 1 && (lg >= 0 || hp == 0);
    const int ts = base + lg + 1;
    const bool tk = has_tail && ng - ts >= min_len;
    const bool th = tk && ni > 0 && ts - li > mw;
    GdSum r;
    r.nk = ni + (tk ? 1 : 0);
    r.f = ni > 0 ? fi : (tk ? ts : GD_FAR);
    r.le = tk ? ng : li;
    r.h = hi + (th ? 1 : 0);
    r.lh = th ? ts : lhi;
    return r;
}

__global__ __launch_bounds__(GD_THREADS) void gd_rows_kernel(const int* __restrict__ lengths, int n, int ntiles, int min_len, int mw, int K,
                                                             int* __restrict__ tab, long tiles_total, int* __restrict__ count,
                                                             int* __restrict__ start, int* __restrict__ length) {
    __shared__ int sh[GD_THREADS];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int len = gd_row_len(lengths, b, n);
    const int per = (ntiles + GD_THREADS - 1) / GD_THREADS;                 // consecutive tiles per thread
    const int t0 = tid * per < ntiles ? tid * per : ntiles, t1 = t0 + per < ntiles ? t0 + per : ntiles;
    const long row = (long)b * ntiles;
    int total;
    // A: the first good index behind every tile
    int mn = GD_FAR;
    for (int t = t0; t < t1; ++t) {
        const int fg = tab[GD_FG * tiles_total + row + t];
        if (fg < GD_TILE) {
            mn = t * GD_TILE + fg;
            break;
        }
    }
    int run = gd_block_scan(mn, GD_FAR, OpMin(), sh, GD_THREADS - 1 - tid, &total);
    for (int t = t1 - 1; t >= t0; --t) {
        tab[GD_NG * tiles_total + row + t] = run == GD_FAR ? len : run;   // damaged to the end of the padded row: then len = ntiles GD_TILE
        const int fg = tab[GD_FG * tiles_total + row + t];
        if (fg < GD_TILE) run = t * GD_TILE + fg;
    }
    // B: the end of the last kept run in front of every tile, and with it the tile's heads
    int last = GD_NONE;
    for (int t = t0; t < t1; ++t) {
        const GdSum s = gd_tile_sum(tab, tiles_total, row + t, t * GD_TILE, tab[GD_NG * tiles_total + row + t], min_len, mw);
        if (s.nk > 0) last = s.le;
    }
    int row_last_end;
    run = gd_block_scan(last, GD_NONE, OpMax(), sh, tid, &row_last_end);
    int hsum = 0, lmax = GD_NONE;
    for (int t = t0; t < t1; ++t) {
        const GdSum s = gd_tile_sum(tab, tiles_total, row + t, t * GD_TILE, tab[GD_NG * tiles_total + row + t], min_len, mw);
        tab[GD_PREV * tiles_total + row + t] = run;
        const bool fh = s.nk > 0 && (run == GD_NONE || s.f - run > mw);
        const int heads = s.h + (fh ? 1 : 0), lh = s.lh != GD_NONE ? s.lh : (fh ? s.f : GD_NONE);
        tab[GD_HEADS * tiles_total + row + t] = heads;
        tab[GD_CUR * tiles_total + row + t] = lh;                           // the tile's own last head; C turns it into the carry
        hsum += heads;
        lmax = lh > lmax ? lh : lmax;
        if (s.nk > 0) run = s.le;
    }
    // C: where the tile's runs go, and the run that is open at its head
    int cnt, row_last_head;
    int off = gd_block_scan(hsum, 0, OpAdd(), sh, tid, &cnt);
    int cur = gd_block_scan(lmax, GD_NONE, OpMax(), sh, tid, &row_last_head);
    for (int t = t0; t < t1; ++t) {
        tab[GD_OFF * tiles_total + row + t] = off;
        off += tab[GD_HEADS * tiles_total + row + t];
        const int lh = tab[GD_CUR * tiles_total + row + t];
        tab[GD_CUR * tiles_total + row + t] = cur;
        cur = lh > cur ? lh : cur;
    }
    // the row's own outputs: launch 3 writes start[k] for k < min(count, K) and length[k] for k < count - 1
    if (tid == 0) {
        count[b] = cnt;
        if (cnt >= 1 && cnt <= K) length[(long)b * K + cnt - 1] = row_last_end - row_last_head;
    }
    for (int k = (cnt < K ? cnt : K) + tid; k < K; k += GD_THREADS) {
        start[(long)b * K + k] = 0;
        length[(long)b * K + k] = 0;
    }
}

__global__ __launch_bounds__(GD_THREADS) void gd_emit_kernel(const unsigned long long* __restrict__ mask, const int* __restrict__ tab,
                                                             long tiles_total, int ntiles, int min_len, int mw, int K, int* __restrict__ start,
                                                             int* __restrict__ length) {
    const int lane = threadIdx.x & 63;
    const long at = (long)blockIdx.x * GD_WAVES + (threadIdx.x >> 6);
    if (at >= tiles_total) return;                                          // whole waves from here on
    const int heads = tab[GD_HEADS * tiles_total + at], off = tab[GD_OFF * tiles_total + at];
    if (heads == 0 || off > K) return;                                      // nothing begins here, or nothing of it is within the first K
    const int b = (int)(at / ntiles), t = (int)(at - (long)b * ntiles), base = t * GD_TILE;
    const unsigned long long m = mask[at * GD_WORDS + lane];
    const GdLane L = gd_lane(m, tab[GD_HP * tiles_total + at], lane);
    const int nz = L.nz_rel == GD_FAR ? tab[GD_NG * tiles_total + at] : base + L.nz_rel;
    const int w0 = base + 64 * lane;
    const GdSum s = gd_word_sum(m, L.prev, w0, nz, min_len, mw);
    const int in_front = gd_wave_prefix(s.le, GD_NONE, OpMax(), lane), tile_prev = tab[GD_PREV * tiles_total + at];
    const int carry = in_front > tile_prev ? in_front : tile_prev;
    const bool fh = s.nk > 0 && (carry == GD_NONE || s.f - carry > mw);
    const int idx = off + gd_wave_prefix(s.h + (fh ? 1 : 0), 0, OpAdd(), lane);
    const int lh = gd_wave_prefix(s.lh != GD_NONE ? s.lh : (fh ? s.f : GD_NONE), GD_NONE, OpMax(), lane), tile_cur = tab[GD_CUR * tiles_total + at];
    if (s.nk > 0)
        gd_word_emit(m, L.prev, w0, nz, min_len, mw, carry, lh > tile_cur ? lh : tile_cur, idx, K, start + (long)b * K, length + (long)b * K);
}

inline bool gd_rule_ok(long stride, long n, float threshold, float clip, int min_len, int merge_within) {
    return stride >= n && min_len >= 1 && merge_within >= 0 && threshold >= 0.f && clip >= 0.f;      // a NaN fails both comparisons
}

inline unsigned gd_bits(float v) {
    unsigned u;
    std::memcpy(&u, &v, sizeof(u));
    return u;
}

}  // namespace

extern "C" long viai_gap_detect_ws_bytes(int B, long n, int K) {
    if (!gd_shape_ok(B, n, K)) return 0;
    return (long)B * gd_tiles(n) * (long)(GD_WORDS * sizeof(unsigned long long) + GD_FIELDS * sizeof(int));
}

extern "C" int viai_gap_detect(const float* wav, const int* lengths, long stride, int B, long n, float threshold, float clip, int min_len,
                               int merge_within, int K, int* count, int* start, int* length, void* ws, void* stream) {
    if (wav == nullptr || count == nullptr || start == nullptr || length == nullptr || ws == nullptr || !gd_shape_ok(B, n, K) ||
        !gd_rule_ok(stride, n, threshold, clip, min_len, merge_within) || (reinterpret_cast<uintptr_t>(wav) & 3) != 0 ||
        (reinterpret_cast<uintptr_t>(ws) & 7) != 0)
        return (int)hipErrorInvalidValue;
    const long ntiles = gd_tiles(n), tiles_total = (long)B * ntiles;
    unsigned long long* mask = static_cast<unsigned long long*>(ws);
    int* tab = reinterpret_cast<int*>(mask + tiles_total * GD_WORDS);
    const unsigned thr_bits = gd_bits(std::fabs(threshold)), hi_bits = clip > 0.f ? gd_bits(clip) : 0x7f800000u;
    hipStream_t st = (hipStream_t)stream;
    VIAI_LAUNCH(gd_mask_kernel, dim3((unsigned)tiles_total), dim3(GD_THREADS), 0, st, wav, lengths, stride, (int)n, (int)ntiles, thr_bits, hi_bits,
                min_len, merge_within, mask, tab, tiles_total);
    return viai_gd_launch_runs(lengths, (int)n, (int)ntiles, min_len, merge_within, K, mask, tab, tiles_total, count, start, length, st);
}

// launches 2 and 3, for every caller that has written a mask and its launch-1 summaries (viai_gap_runs.h); the status covers the caller's
// earlier launches from this translation unit as well
int viai_gd_launch_runs(const int* lengths, int n, int ntiles, int min_len, int merge_within, int K, const unsigned long long* mask, int* tab,
                        long tiles_total, int* count, int* start, int* length, hipStream_t st) {
    const int B = (int)(tiles_total / ntiles);
    VIAI_LAUNCH(gd_rows_kernel, dim3((unsigned)B), dim3(GD_THREADS), 0, st, lengths, n, ntiles, min_len, merge_within, K, tab, tiles_total, count,
                start, length);
    VIAI_LAUNCH(gd_emit_kernel, dim3((unsigned)((tiles_total + GD_WAVES - 1) / GD_WAVES)), dim3(GD_THREADS), 0, st, mask, tab, tiles_total, ntiles,
                min_len, merge_within, K, start, length);
    return viai_launch_status();
}

// The rule stated sample by sample, every pointer in host memory: no tiles, no words, no carries.
extern "C" int viai_gap_detect_host(const float* wav, const int* lengths, long stride, int B, long n, float threshold, float clip, int min_len,
                                    int merge_within, int K, int* count, int* start, int* length) {
    if (wav == nullptr || count == nullptr || start == nullptr || length == nullptr || !gd_shape_ok(B, n, K) ||
        !gd_rule_ok(stride, n, threshold, clip, min_len, merge_within))
        return (int)hipErrorInvalidValue;
    for (int b = 0; b < B; ++b) {
        const float* x = wav + (long)b * stride;
        long len = lengths != nullptr ? (long)lengths[b] : n;
        len = len < 0 ? 0 : (len > n ? n : len);
        auto damaged = [&](long i) {
            const float a = std::fabs(x[i]);
            return !std::isfinite(x[i]) || a <= threshold || (clip > 0.f && a >= clip);
        };
        count[b] = gd_runs_host(len, damaged, min_len, merge_within, K, start + (long)b * K, length + (long)b * K);
    }
    return 0;
}
