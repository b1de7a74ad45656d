// The join between the mel generator and the WaveNet vocoder (gfx950): which frames a gap in SAMPLES damages, the waveform moved onto the
// vocoder's frame grid with the gap silenced, and the conditioning selected from the real and the generated mel.  Contracts: include/viai_hip.h,
// derivation: DESIGN.md 11.2g.  Three streaming kernels, one launch each: no LDS, no atomics, no arithmetic on a sample or mel value (values move as
// 32-bit words, so NaN payloads and signed zeros survive).  An output of `total` words is walked as
//     [ head scalars | nvec float4 groups | tail scalars ],    head = words up to the output's first 16-byte boundary (0 for a torch allocation),
// item i < nvec being group i and the items behind it the head and tail words one by one.
#include "viai_common.h"
#include "viai_internal.h"

namespace {

struct ij_split {
    int head;
    long nvec;
    int tail;
};

inline ij_split ij_make(const void* out, long total) {
    ij_split s;
    long head = (long)(((16 - ((uintptr_t)out & 15)) & 15) / 4);
    if (head > total) head = total;
    s.head = (int)head;
    s.nvec = (total - head) / 4;
    s.tail = (int)(total - head - 4 * s.nvec);
    return s;
}

// word index of scalar item k (0 <= k < head + tail)
__device__ inline long ij_scalar(long k, int head, long nvec) { return k < head ? k : (long)head + 4 * nvec + (k - head); }

// ---- mask[b][j] = 0 where frame j's window [j hop, j hop + fft) meets the gap [a0[b], a1[b]), else 1
__device__ inline float gfm_value(int a0, int a1, long j, int fft, int hop) {
    const long lo = j * hop;
    return (a0 < a1 && lo < a1 && lo + fft > a0) ? 0.f : 1.f;
}

__global__ __launch_bounds__(256) void gap_frame_mask_kernel(const int* __restrict__ a0, const int* __restrict__ a1, float* __restrict__ mask, int frames,
                                                             int fft, int hop, int head, long nvec, int tail) {
    const long items = nvec + head + tail;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < items; i += (long)gridDim.x * 256L) {
        if (i < nvec) {
            const long e0 = head + 4 * i;
            long b = e0 / frames;
            long j = e0 - b * frames;
            float v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                v[k] = gfm_value(a0[b], a1[b], j, fft, hop);
                if (++j == frames) { j = 0; ++b; }
            }
            *reinterpret_cast<f32x4*>(mask + e0) = f32x4{v[0], v[1], v[2], v[3]};
        } else {
            const long e = ij_scalar(i - nvec, head, nvec);
            const long b = e / frames;
            mask[e] = gfm_value(a0[b], a1[b], e - b * frames, fft, hop);
        }
    }
}

// ---- out (B, n + lpad): zeros in front of the clip and inside [a0[b], a1[b]), the clip's words elsewhere.
// VEC: n, lpad multiples of 4 and wav 16-byte aligned -- a group then lies in one row, on one side of lpad, and its source is aligned too.
__device__ inline unsigned wa_value(const unsigned* __restrict__ wav, int a0, int a1, long b, long a, int n, int lpad) {
    return (a < lpad || (a >= a0 && a < a1)) ? 0u : wav[b * n + (a - lpad)];
}

template <bool VEC>
__global__ __launch_bounds__(256) void wav_align_kernel(const unsigned* __restrict__ wav, const int* __restrict__ a0, const int* __restrict__ a1,
                                                        unsigned* __restrict__ out, int n, int lpad, int head, long nvec, int tail) {
    const long items = nvec + head + tail;
    const long row = (long)n + lpad;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < items; i += (long)gridDim.x * 256L) {
        if (i < nvec) {
            const long e0 = head + 4 * i;
            long b = e0 / row;
            long a = e0 - b * row;
            u32x4 v = u32x4{0u, 0u, 0u, 0u};
            if (VEC) {                                             // head == 0 here: out is aligned like wav
                const int g0 = a0[b], g1 = a1[b];
                if (a >= lpad) {
                    v = *reinterpret_cast<const u32x4*>(wav + b * n + (a - lpad));
                    if (a + 0 >= g0 && a + 0 < g1) v.x = 0u;
                    if (a + 1 >= g0 && a + 1 < g1) v.y = 0u;
                    if (a + 2 >= g0 && a + 2 < g1) v.z = 0u;
                    if (a + 3 >= g0 && a + 3 < g1) v.w = 0u;
                }
            } else {
                unsigned w[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    w[k] = wa_value(wav, a0[b], a1[b], b, a, n, lpad);
                    if (++a == row) { a = 0; ++b; }
                }
                v = u32x4{w[0], w[1], w[2], w[3]};
            }
            *reinterpret_cast<u32x4*>(out + e0) = v;
        } else {
            const long e = ij_scalar(i - nvec, head, nvec);
            const long b = e / row;
            out[e] = wa_value(wav, a0[b], a1[b], b, e - b * row, n, lpad);
        }
    }
}

// ---- c[b][f][t] = mask[b][t] != 0 ? real[b][f][t] : fake[b][f][t]; the three tensors share one flat index (FT = F T words per stream).
// VEC: real + head and fake + head are 16-byte aligned, i.e. the inputs are aligned like c.
template <bool VEC>
__global__ __launch_bounds__(256) void mel_compose_kernel(const unsigned* __restrict__ real, const unsigned* __restrict__ fake, const float* __restrict__ mask,
                                                          unsigned* __restrict__ c, long FT, int T, int head, long nvec, int tail) {
    const long items = nvec + head + tail;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < items; i += (long)gridDim.x * 256L) {
        if (i < nvec) {
            const long e0 = head + 4 * i;
            long b = e0 / FT;
            const long r = e0 - b * FT;
            int t = (int)(r % T);
            long left = FT - r;                                    // words of stream b from e0 on
            bool keep[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                keep[k] = mask[b * T + t] != 0.f;
                if (++t == T) t = 0;
                if (--left == 0) { left = FT; ++b; }               // FT is a multiple of T: t is 0 here as well
            }
            u32x4 x, y;
            if (VEC) {
                x = *reinterpret_cast<const u32x4*>(real + e0);
                y = *reinterpret_cast<const u32x4*>(fake + e0);
            } else {
                x = u32x4{real[e0], real[e0 + 1], real[e0 + 2], real[e0 + 3]};
                y = u32x4{fake[e0], fake[e0 + 1], fake[e0 + 2], fake[e0 + 3]};
            }
            *reinterpret_cast<u32x4*>(c + e0) = u32x4{keep[0] ? x.x : y.x, keep[1] ? x.y : y.y, keep[2] ? x.z : y.z, keep[3] ? x.w : y.w};
        } else {
            const long e = ij_scalar(i - nvec, head, nvec);
            const long b = e / FT;
            const int t = (int)((e - b * FT) % T);
            c[e] = mask[b * T + t] != 0.f ? real[e] : fake[e];
        }
    }
}

inline bool ij_word_aligned(const void* p) { return ((uintptr_t)p & 3) == 0; }
inline bool ij_vec_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int viai_gap_frame_mask(const int* a0, const int* a1, float* mask, int B, int frames, int fft, int hop, void* stream) {
    if (B < 1 || frames < 1 || fft < 1 || hop < 1 || a0 == nullptr || a1 == nullptr || mask == nullptr || !ij_word_aligned(mask))
        return (int)hipErrorInvalidValue;
    const ij_split s = ij_make(mask, (long)B * frames);
    VIAI_LAUNCH(gap_frame_mask_kernel, dim3(viai_ew_blocks(s.nvec + s.head + s.tail)), dim3(256), 0, (hipStream_t)stream, a0, a1, mask, frames, fft, hop, s.head,
                s.nvec, s.tail);
    return viai_launch_status();
}

extern "C" int viai_wav_align(const float* wav, const int* a0, const int* a1, float* out, int B, int n, int lpad, void* stream) {
    if (B < 1 || n < 1 || lpad < 0 || wav == nullptr || a0 == nullptr || a1 == nullptr || out == nullptr || !ij_word_aligned(wav) || !ij_word_aligned(out))
        return (int)hipErrorInvalidValue;
    const ij_split s = ij_make(out, (long)B * ((long)n + lpad));
    const unsigned* w = reinterpret_cast<const unsigned*>(wav);
    unsigned* o = reinterpret_cast<unsigned*>(out);
    const dim3 grid(viai_ew_blocks(s.nvec + s.head + s.tail));
    if (n % 4 == 0 && lpad % 4 == 0 && s.head == 0 && ij_vec_aligned(wav))
        VIAI_LAUNCH(wav_align_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, w, a0, a1, o, n, lpad, s.head, s.nvec, s.tail);
    else
        VIAI_LAUNCH(wav_align_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, w, a0, a1, o, n, lpad, s.head, s.nvec, s.tail);
    return viai_launch_status();
}

extern "C" int viai_mel_compose(const float* real, const float* fake, const float* mask, float* c, int B, int F, int T, void* stream) {
    if (B < 1 || F < 1 || T < 1 || real == nullptr || fake == nullptr || mask == nullptr || c == nullptr || !ij_word_aligned(real) ||
        !ij_word_aligned(fake) || !ij_word_aligned(c))
        return (int)hipErrorInvalidValue;
    const long FT = (long)F * T;
    const ij_split s = ij_make(c, (long)B * FT);
    const unsigned* x = reinterpret_cast<const unsigned*>(real);
    const unsigned* y = reinterpret_cast<const unsigned*>(fake);
    unsigned* o = reinterpret_cast<unsigned*>(c);
    const dim3 grid(viai_ew_blocks(s.nvec + s.head + s.tail));
    if (ij_vec_aligned(x + s.head) && ij_vec_aligned(y + s.head))
        VIAI_LAUNCH(mel_compose_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, x, y, mask, o, FT, T, s.head, s.nvec, s.tail);
    else
        VIAI_LAUNCH(mel_compose_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, x, y, mask, o, FT, T, s.head, s.nvec, s.tail);
    return viai_launch_status();
}
