// WaveNet training batches (gfx950): `collate_fn` of Data_loaders/data_loader_utils.py:209-319 behind the crop plan.  Contract: include/viai_hip.h,
// derivation and figures: DESIGN.md 11.2j.  One entry point, ONE launch per batch; the blocks of a row are, along grid x,
//     signal    1024 samples each: the cropped row -> y (int64 targets) and classes (int32), or the float input, zero padded to T_out
//     one-hot   256 samples each, all K classes: the tile's classes staged in LDS, thread (k, t4) writes float4(cls[t .. t+3] == k)
//     mel       32 frames x 32 bands each: (frames, D) -> (D, L_out) through a padded LDS tile, zero filled past the row's frames
// Every store address is a function of (b, k or d, t) alone -- never of a class read from memory -- and every source index is below
// (start + frames) * hop resp. (start + frames) * D of its row.  No atomics: each output element has one writer, the same bits on every run.
#include <climits>
#include <cstdint>

#include "viai_common.h"
#include "viai_internal.h"

namespace {

constexpr int VB_NT = 256;                   // threads of a block
constexpr int VB_SIG = 4 * VB_NT;            // samples of a signal block: four per thread
constexpr int VB_OH_T = 256;                 // samples of a one-hot tile: 64 float4 columns x 4 class rows per pass
constexpr int VB_TILE = 32;                  // frames and bands of a transpose tile; the pitch of VB_TILE + 1 words puts the 32 frames a
                                             // half-wave reads for one band on 32 different LDS banks (ds_read_b32 banks are (a / 4) % 32)

struct VbRow {
    int start, frames;                       // first frame of the crop, frames kept (clamped to [0, L_out])
    long len;                                // frames * hop: samples kept
};

__device__ __forceinline__ VbRow vb_row(const int* __restrict__ start, const int* __restrict__ frames, int b, int hop, int L_out) {
    VbRow r;
    r.start = start[b] < 0 ? 0 : start[b];
    const int f = frames[b];
    r.frames = f < 0 ? 0 : (f > L_out ? L_out : f);
    r.len = (long)r.frames * hop;
    return r;
}

// four consecutive samples of the cropped row, `fill` past its end.  vec: the row's first kept sample is 16-byte aligned and hop % 4 == 0, so a
// group of four lies wholly inside or wholly outside the row.
__device__ __forceinline__ u32x4 vb_load4(const unsigned* __restrict__ src, long t0, long len, bool vec, unsigned fill) {
    u32x4 w = {fill, fill, fill, fill};
    if (vec) {
        if (t0 + 4 <= len) w = *reinterpret_cast<const u32x4*>(src + t0);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (t0 + k < len) w[k] = src[t0 + k];
    }
    return w;
}

__global__ __launch_bounds__(VB_NT) void voc_collate_kernel(const void* const* __restrict__ sig_ptr, const float* const* __restrict__ mel_ptr,
                                                            const int* __restrict__ start, const int* __restrict__ frames, int hop, int D, int mode, int K,
                                                            long T_out, int L_out, long long* __restrict__ y, int* __restrict__ classes,
                                                            float* __restrict__ x, float* __restrict__ c, int n_sig, int n_oh, int out_vec) {
    __shared__ int cls[VB_OH_T];
    __shared__ float tile[VB_TILE][VB_TILE + 1];
    const int b = blockIdx.y, tid = threadIdx.x;
    const VbRow r = vb_row(start, frames, b, hop, L_out);
    int blk = blockIdx.x;                                                           // (every branch below is uniform over the block)
    if (blk < n_sig + n_oh) {
        const unsigned* src = static_cast<const unsigned*>(sig_ptr[b]) + (long)r.start * hop;
        const bool src_vec = (hop & 3) == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0;
        if (blk < n_sig) {
            // ---- signal: y / classes (mode 0) or the float row (modes 1, 2: y holds floats, [B][T_out])
            const long t0 = (long)blk * VB_SIG + 4L * tid;
            if (t0 >= T_out) return;
            const u32x4 w = vb_load4(src, t0, r.len, src_vec, 0u);
            const size_t o = (size_t)b * (size_t)T_out + (size_t)t0;
            if (mode == VIAI_UTT_MULAW_QUANTIZE) {
                if (out_vec) {                                                          // T_out % 4 == 0: the group is whole
                    long long* yo = y + o;
                    typedef long long i64x2 __attribute__((ext_vector_type(2)));
                    *reinterpret_cast<i64x2*>(yo) = i64x2{(long long)(int)w[0], (long long)(int)w[1]};
                    *reinterpret_cast<i64x2*>(yo + 2) = i64x2{(long long)(int)w[2], (long long)(int)w[3]};
                    if (classes != nullptr) *reinterpret_cast<u32x4*>(classes + o) = w;
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (t0 + k < T_out) {
                            y[o + k] = (long long)(int)w[k];
                            if (classes != nullptr) classes[o + k] = (int)w[k];
                        }
                }
            } else {
                unsigned* fo = reinterpret_cast<unsigned*>(y) + o;
                if (out_vec) {
                    *reinterpret_cast<u32x4*>(fo) = w;
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (t0 + k < T_out) fo[k] = w[k];
                }
            }
            return;
        }
        // ---- one-hot: x [B][K][T_out].  A class outside [0, K) -- and the -1 staged past the row's end -- equals no k: a zero column.
        blk -= n_sig;
        const long tb = (long)blk * VB_OH_T;
        {
            const long t = tb + tid;                                                    // VB_OH_T == VB_NT: one class per thread
            cls[tid] = t < r.len ? (int)src[t] : -1;
        }
        __syncthreads();
        const int t4 = tid & 63, k0 = tid >> 6;
        const long t0 = tb + 4L * t4;
        if (t0 >= T_out) return;
        const int c0 = cls[4 * t4], c1 = cls[4 * t4 + 1], c2 = cls[4 * t4 + 2], c3 = cls[4 * t4 + 3];
        float* xo = x + (size_t)b * (size_t)K * (size_t)T_out + (size_t)t0;
        for (int k = k0; k < K; k += VB_NT / 64) {
            const f32x4 v = {c0 == k ? 1.f : 0.f, c1 == k ? 1.f : 0.f, c2 == k ? 1.f : 0.f, c3 == k ? 1.f : 0.f};
            float* p = xo + (size_t)k * (size_t)T_out;
            if (out_vec) {
                *reinterpret_cast<f32x4*>(p) = v;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (t0 + j < T_out) p[j] = v[j];
            }
        }
        return;
    }
    // ---- mel: (frames, D) -> c [B][D][L_out].  Reads run along D, writes along the frames.
    blk -= n_sig + n_oh;
    const int nd = (D + VB_TILE - 1) / VB_TILE;
    const int f0 = (blk / nd) * VB_TILE, d0 = (blk % nd) * VB_TILE;
    const int tx = tid & (VB_TILE - 1), ty = tid >> 5;                                  // 32 x 8
    const float* m = mel_ptr[b] + (size_t)r.start * (size_t)D;
#pragma unroll
    for (int i = ty; i < VB_TILE; i += VB_NT / VB_TILE) {                               // (a frame past the row's own is not read: zero)
        const int f = f0 + i, d = d0 + tx;
        tile[i][tx] = (f < r.frames && d < D) ? m[(size_t)f * (size_t)D + d] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int i = ty; i < VB_TILE; i += VB_NT / VB_TILE) {
        const int d = d0 + i, f = f0 + tx;
        if (d < D && f < L_out) c[((size_t)b * (size_t)D + d) * (size_t)L_out + f] = tile[tx][i];
    }
}

inline bool voc_mode_ok(int mode) { return mode == VIAI_UTT_MULAW_QUANTIZE || mode == VIAI_UTT_MULAW || mode == VIAI_UTT_RAW; }

}  // namespace

extern "C" int viai_voc_collate(const void* const* sig_ptr, const float* const* mel_ptr, const int* start, const int* frames, int B, int hop, int D, int mode,
                                int K, long T_out, int L_out, long long* y, int* classes, float* x, float* c, void* stream) {
    if (sig_ptr == nullptr || start == nullptr || frames == nullptr || y == nullptr || B < 1 || B > 65535 || hop < 1 || !voc_mode_ok(mode) ||
        (mode == VIAI_UTT_MULAW_QUANTIZE && K < 2) || (x != nullptr && K % 4 != 0) || (mel_ptr != nullptr && D < 1) ||
        (mel_ptr != nullptr) != (c != nullptr) || T_out < hop || T_out % hop != 0 || T_out > (long)INT_MAX || L_out < 1 ||
        (long)L_out * hop != T_out)
        return (int)hipErrorInvalidValue;
    const bool onehot = mode == VIAI_UTT_MULAW_QUANTIZE && x != nullptr;
    const bool mel = mel_ptr != nullptr;
    // 16-byte stores need every output row to start on a 16-byte boundary: aligned bases and T_out % 4 == 0 (y: 8 T_out bytes a row)
    const uintptr_t bases = (uintptr_t)y | (uintptr_t)classes | (onehot ? (uintptr_t)x : 0);
    const int out_vec = (bases & 15) == 0 && T_out % 4 == 0;
    if (((uintptr_t)y & (mode == VIAI_UTT_MULAW_QUANTIZE ? 7 : 3)) != 0 || ((uintptr_t)classes & 3) != 0 || ((uintptr_t)x & 3) != 0 || ((uintptr_t)c & 3) != 0)
        return (int)hipErrorInvalidValue;
    const long n_sig = (T_out + VB_SIG - 1) / VB_SIG;
    const long n_oh = onehot ? (T_out + VB_OH_T - 1) / VB_OH_T : 0;
    const long n_mel = mel ? (long)((L_out + VB_TILE - 1) / VB_TILE) * ((D + VB_TILE - 1) / VB_TILE) : 0;
    if (n_sig + n_oh + n_mel > (long)INT_MAX) return (int)hipErrorInvalidValue;
    VIAI_LAUNCH(voc_collate_kernel, dim3((unsigned)(n_sig + n_oh + n_mel), (unsigned)B), dim3(VB_NT), 0, (hipStream_t)stream, sig_ptr, mel_ptr, start, frames,
                hop, D, mode, K, T_out, L_out, y, classes, x, c, (int)n_sig, (int)n_oh, out_vec);
    return viai_launch_status();
}
