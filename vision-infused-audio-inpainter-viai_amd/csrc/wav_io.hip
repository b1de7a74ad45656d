// WAV in, WAV out (gfx950): interleaved little-endian PCM bytes <-> planar fp32, and in-place patching of the bytes of detected gaps.
// Contract and rule: include/viai_hip.h; the per-sample arithmetic: viai_pcm_rule.h (shared with the host mirrors at the end of this file);
// layout, choices and measured rate: DESIGN.md 11.2p.
//
//   pcm_decode_kernel   one block per TILE of 1024 frames.  The tile's bytes come into LDS with 16-byte loads (a tile starts 16-byte aligned in
//                       the stream for every frame size because TILE is a multiple of 16; the tail of the last tile byte by byte).  Thread t then
//                       owns frames 4 t .. 4 t + 3: per channel it reads its four samples from LDS and writes them with one 16-byte store.
//   pcm_peak_kernel     one block per tile: max |x| over its finite samples, as the bits of a non-negative float (they order like integers).
//   pcm_encode_kernel   the transpose the other way round: 16-byte loads of four frames of a plane, samples into LDS at their byte position,
//                       16-byte stores of the tile's bytes.  With normalize every block first takes the maximum of ALL partials, so there is no
//                       atomic and no third launch; to keep that at a few hundred MB of L2 reads for the longest clips the grid is capped and a
//                       block walks tiles blockIdx.x, blockIdx.x + gridDim.x, ...
//   pcm_patch_kernel    grid.y = (channel, gap index); a lane encodes one sample of the run and stores exactly its bytes.
//
// LDS layout: the byte stream as dwords.  Thread t reads four frames, fb = C bps dwords, so the lane stride is fb dwords.  An odd fb (U8 and S24
// with an odd channel count, 3- and 9-byte frames included) is conflict-free as it stands.  An even fb puts the 32 lanes of a half-wave on
// 32 / gcd(fb, 32) banks (fb = 64, F64 x 8: all on one), so for even fb dword w is stored at w ^ ((w / 32) % 32): row r of 32 dwords moves by r
// banks.  Enumerated over every fb the formats allow (ds_read_b32, 32 banks per half-wave): 1 for fb = 2, 4, 8, 16, 32; 2 for 20, 40, 48, 56,
// 64; 3 for 6, 10, 12, 14, 18, 24, 28 -- against 2 to 32 without it.  The XOR stays inside a 128-byte row: no padding, 64 KiB for F64 x 8.
#include <cstring>

#include "viai_common.h"
#include "viai_pcm_rule.h"

namespace {

constexpr int PCM_TILE = VIAI_PCM_TILE;
constexpr int PCM_THREADS = 256;
constexpr int PCM_MAX_BLOCKS = 2048;                       // encode: 8 blocks on each of 256 CUs
constexpr int PCM_PATCH_BLOCKS = 32;                       // patch: blocks along one run (grid-stride)
static_assert(PCM_TILE == 4 * PCM_THREADS, "a thread owns four frames of the tile");
static_assert(PCM_TILE % 16 == 0 && PCM_TILE * 8 * 8 <= 65536, "tiles start 16-byte aligned; 64 KiB of LDS at most");

template <int FMT> struct PcmBps { static constexpr int v = FMT == VIAI_PCM_U8 ? 1 : FMT == VIAI_PCM_S16 ? 2 : FMT == VIAI_PCM_S24 ? 3 : FMT == VIAI_PCM_F64 ? 8 : 4; };

__device__ __forceinline__ unsigned pcm_swz(unsigned w, unsigned sm) { return w ^ ((w >> 5) & sm); }                        // sm: 31, or 0 for an odd fb
__device__ __forceinline__ unsigned pcm_phys(unsigned a, unsigned sm) { return (pcm_swz(a >> 2, sm) << 2) | (a & 3u); }      // of a byte address

// the raw sample at byte address a of the staged stream; last: the index of the last dword of the stage
template <int BPS>
__device__ __forceinline__ unsigned long long pcm_lds_get(const unsigned* lds, unsigned a, unsigned last, unsigned sm) {
    const unsigned w = a >> 2, sh = 8u * (a & 3u);
    if (BPS == 1) return (lds[pcm_swz(w, sm)] >> sh) & 0xffu;
    if (BPS == 2) return (lds[pcm_swz(w, sm)] >> sh) & 0xffffu;                                               // a is even: inside one dword
    if (BPS == 3) {
        const unsigned lo = lds[pcm_swz(w, sm)], hi = lds[pcm_swz(w + 1 > last ? last : w + 1, sm)];              // hi matters only when a % 4 >= 2
        return ((((unsigned long long)hi << 32) | lo) >> sh) & 0xffffffu;
    }
    if (BPS == 4) return lds[pcm_swz(w, sm)];
    return ((unsigned long long)lds[pcm_swz(w + 1, sm)] << 32) | lds[pcm_swz(w, sm)];
}
template <int BPS>
__device__ __forceinline__ void pcm_lds_put(unsigned* lds, unsigned a, unsigned long long raw, unsigned sm) {
    unsigned char* b = reinterpret_cast<unsigned char*>(lds);
    if (BPS == 1) b[pcm_phys(a, sm)] = (unsigned char)raw;
    if (BPS == 2) *reinterpret_cast<unsigned short*>(b + pcm_phys(a, sm)) = (unsigned short)raw;
    if (BPS == 3) {
        b[pcm_phys(a, sm)] = (unsigned char)raw;
        b[pcm_phys(a + 1, sm)] = (unsigned char)(raw >> 8);
        b[pcm_phys(a + 2, sm)] = (unsigned char)(raw >> 16);
    }
    if (BPS == 4) lds[pcm_swz(a >> 2, sm)] = (unsigned)raw;
    if (BPS == 8) {
        lds[pcm_swz(a >> 2, sm)] = (unsigned)raw;
        lds[pcm_swz((a >> 2) + 1, sm)] = (unsigned)(raw >> 32);
    }
}

// four frames of one plane, of which n >= 1 exist: one 16-byte access where all four exist and the address allows it
__device__ __forceinline__ void pcm_store4(float* p, const float (&v)[4], int n) {
    if (n >= 4 && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
        f32x4 q = {v[0], v[1], v[2], v[3]};
        *reinterpret_cast<f32x4*>(p) = q;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < n) p[k] = v[k];
    }
}
__device__ __forceinline__ void pcm_load4(const float* p, float (&v)[4], int n) {
    if (n >= 4 && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
        const f32x4 q = *reinterpret_cast<const f32x4*>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = k < n ? p[k] : 0.f;
    }
}

__device__ __forceinline__ unsigned pcm_wave_max(unsigned m) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned u = (unsigned)__shfl_xor((int)m, o, 64);
        m = u > m ? u : m;
    }
    return m;
}

template <int FMT>
__global__ __launch_bounds__(PCM_THREADS) void pcm_decode_kernel(const unsigned char* __restrict__ src, int C, long frames, int mono,
                                                                 float* __restrict__ out, long out_stride) {
    extern __shared__ unsigned pcm_lds[];                                   // PCM_TILE C bps bytes
    constexpr int BPS = PcmBps<FMT>::v;
    const int fb = C * BPS, tid = threadIdx.x;
    const unsigned sm = (fb & 1) ? 0u : 31u;
    const long f0 = (long)blockIdx.x * PCM_TILE;                            // < frames: the grid is ceil(frames / TILE)
    const int nf = frames - f0 < PCM_TILE ? (int)(frames - f0) : PCM_TILE;
    const int nbytes = nf * fb, full = nbytes >> 4;
    const unsigned char* __restrict__ g = src + f0 * fb;                    // 16-byte aligned: src is, and TILE fb is a multiple of 16
    for (int q = tid; q < full; q += PCM_THREADS) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(g + 16 * q);
        const unsigned w = 4u * q;                                          // the four dwords stay in one row of 32
        pcm_lds[pcm_swz(w, sm)] = v.x;
        pcm_lds[pcm_swz(w + 1, sm)] = v.y;
        pcm_lds[pcm_swz(w + 2, sm)] = v.z;
        pcm_lds[pcm_swz(w + 3, sm)] = v.w;
    }
    if (tid < (nbytes & 15)) {                                              // the tail of the last tile: no byte behind the stream is read
        const unsigned a = 16u * full + tid;
        reinterpret_cast<unsigned char*>(pcm_lds)[pcm_phys(a, sm)] = g[a];
    }
    __syncthreads();
    const int j = 4 * tid, n = nf - j;
    if (n <= 0) return;
    const unsigned last = (unsigned)(PCM_TILE * fb / 4 - 1);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < C; ++c) {
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            v[k] = k < n ? pcm_decode(FMT, pcm_lds_get<BPS>(pcm_lds, (unsigned)((j + k) * fb + c * BPS), last, sm)) : 0.f;
        if (mono) {
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] = c == 0 ? v[k] : acc[k] + v[k];
        } else {
            pcm_store4(out + (long)c * out_stride + f0 + j, v, n);
        }
    }
    if (mono) {
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] = pcm_mono(acc[k], C);
        pcm_store4(out + f0 + j, acc, n);
    }
}

__global__ __launch_bounds__(PCM_THREADS) void pcm_peak_kernel(const float* __restrict__ wav, long stride, int C, long frames,
                                                               unsigned* __restrict__ ws) {
    __shared__ unsigned red[PCM_THREADS / 64];
    const int tid = threadIdx.x;
    const long f0 = (long)blockIdx.x * PCM_TILE;
    const int nf = frames - f0 < PCM_TILE ? (int)(frames - f0) : PCM_TILE;
    const int j = 4 * tid, n = nf - j;
    unsigned m = 0;
    if (n > 0) {
        for (int c = 0; c < C; ++c) {
            float v[4];
            pcm_load4(wav + (long)c * stride + f0 + j, v, n);               // frames that do not exist read as 0: no change to a maximum
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const unsigned a = __float_as_uint(v[k]) & 0x7fffffffu;
                m = (a < 0x7f800000u && a > m) ? a : m;
            }
        }
    }
    m = pcm_wave_max(m);
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < PCM_THREADS / 64; ++w) m = red[w] > m ? red[w] : m;
        ws[blockIdx.x] = m;
    }
}

template <int FMT>
__global__ __launch_bounds__(PCM_THREADS) void pcm_encode_kernel(const float* __restrict__ wav, long stride, int C, long frames, int normalize,
                                                                 unsigned char* __restrict__ dst, const unsigned* __restrict__ ws, long ntiles) {
    extern __shared__ unsigned pcm_lds[];
    constexpr int BPS = PcmBps<FMT>::v;
    const int fb = C * BPS, tid = threadIdx.x;
    const unsigned sm = (fb & 1) ? 0u : 31u;
    float scale = 0.f;
    if (normalize) {                                                        // block-uniform
        unsigned m = 0;
        for (long i = tid; i < ntiles; i += PCM_THREADS) {
            const unsigned u = ws[i];
            m = u > m ? u : m;
        }
        m = pcm_wave_max(m);
        if ((tid & 63) == 0) pcm_lds[tid >> 6] = m;                         // the stage is free here: no static LDS beside 64 KiB of it
        __syncthreads();
        for (int w = 0; w < PCM_THREADS / 64; ++w) m = pcm_lds[w] > m ? pcm_lds[w] : m;
        __syncthreads();                                                    // the stage is written next
        scale = pcm_norm_scale(__uint_as_float(m));
    }
    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long f0 = tile * PCM_TILE;
        const int nf = frames - f0 < PCM_TILE ? (int)(frames - f0) : PCM_TILE;
        const int nbytes = nf * fb, full = nbytes >> 4;
        const int j = 4 * tid, n = nf - j;
        if (n > 0) {
            for (int c = 0; c < C; ++c) {
                float v[4];
                pcm_load4(wav + (long)c * stride + f0 + j, v, n);
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k < n)
                        pcm_lds_put<BPS>(pcm_lds, (unsigned)((j + k) * fb + c * BPS), normalize ? pcm_encode_norm(v[k], scale) : pcm_encode(FMT, v[k]), sm);
            }
        }
        __syncthreads();
        unsigned char* __restrict__ g = dst + f0 * fb;
        for (int q = tid; q < full; q += PCM_THREADS) {
            const unsigned w = 4u * q;
            u32x4 v;
            v.x = pcm_lds[pcm_swz(w, sm)];
            v.y = pcm_lds[pcm_swz(w + 1, sm)];
            v.z = pcm_lds[pcm_swz(w + 2, sm)];
            v.w = pcm_lds[pcm_swz(w + 3, sm)];
            *reinterpret_cast<u32x4*>(g + 16 * q) = v;
        }
        if (tid < (nbytes & 15)) {                                          // the tail of the last tile: no byte behind the stream is written
            const unsigned a = 16u * full + tid;
            g[a] = reinterpret_cast<const unsigned char*>(pcm_lds)[pcm_phys(a, sm)];
        }
        __syncthreads();                                                    // the next tile overwrites the stage
    }
}

__global__ __launch_bounds__(PCM_THREADS) void pcm_patch_kernel(const float* __restrict__ wav, long stride, int C, long frames, int fmt,
                                                                const int* __restrict__ count, const int* __restrict__ start,
                                                                const int* __restrict__ length, int K, unsigned char* __restrict__ dst) {
    const int c = blockIdx.y / K, k = blockIdx.y - c * K;                   // grid.y = C K
    if (k >= count[c]) return;
    long s = start[(long)c * K + k], e = s + (long)length[(long)c * K + k];
    s = s < 0 ? 0 : s;
    e = e > frames ? frames : e;
    const int bps = pcm_bytes(fmt);
    for (long i = s + (long)blockIdx.x * PCM_THREADS + threadIdx.x; i < e; i += (long)gridDim.x * PCM_THREADS) {
        const unsigned long long raw = pcm_encode(fmt, wav[(long)c * stride + i]);
        unsigned char* p = dst + (i * C + c) * bps;
        const uintptr_t at = reinterpret_cast<uintptr_t>(p);
        // a store is exactly the sample where its address allows, bytes otherwise: never wider than the sample
        if (bps == 2 && (at & 1) == 0) {
            *reinterpret_cast<unsigned short*>(p) = (unsigned short)raw;
        } else if (bps == 4 && (at & 3) == 0) {
            *reinterpret_cast<unsigned*>(p) = (unsigned)raw;
        } else if (bps == 8 && (at & 7) == 0) {
            *reinterpret_cast<unsigned long long*>(p) = raw;
        } else {
            for (int b = 0; b < bps; ++b) p[b] = (unsigned char)(raw >> (8 * b));
        }
    }
}

inline long pcm_tiles(long frames) { return (frames + PCM_TILE - 1) / PCM_TILE; }
inline bool pcm_shape_ok(int fmt, int C, long frames) {
    return pcm_bytes(fmt) > 0 && C >= 1 && C <= 8 && frames >= 0 && frames <= 0x7fffffffL * PCM_TILE;
}
inline bool pcm_aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

inline unsigned long long pcm_host_get(const unsigned char* p, int bps) {
    unsigned long long raw = 0;
    for (int b = 0; b < bps; ++b) raw |= (unsigned long long)p[b] << (8 * b);
    return raw;
}
inline void pcm_host_put(unsigned char* p, int bps, unsigned long long raw) {
    for (int b = 0; b < bps; ++b) p[b] = (unsigned char)(raw >> (8 * b));
}

}  // namespace

#define PCM_BY_FORMAT(fmt, LAUNCH)                          \
    switch (fmt) {                                          \
    case VIAI_PCM_U8: LAUNCH(VIAI_PCM_U8); break;           \
    case VIAI_PCM_S16: LAUNCH(VIAI_PCM_S16); break;         \
    case VIAI_PCM_S24: LAUNCH(VIAI_PCM_S24); break;         \
    case VIAI_PCM_S32: LAUNCH(VIAI_PCM_S32); break;         \
    case VIAI_PCM_F32: LAUNCH(VIAI_PCM_F32); break;         \
    default: LAUNCH(VIAI_PCM_F64); break;                   \
    }

extern "C" int viai_pcm_decode(const unsigned char* src, int fmt, int channels, long frames, int mono, float* out, long out_stride, void* stream) {
    if (src == nullptr || out == nullptr || !pcm_shape_ok(fmt, channels, frames) || out_stride < frames || !pcm_aligned(src, 16) ||
        !pcm_aligned(out, 4))
        return (int)hipErrorInvalidValue;
    if (frames == 0) return 0;
    const size_t lds = (size_t)PCM_TILE * channels * pcm_bytes(fmt);
    const dim3 grid((unsigned)pcm_tiles(frames));
    hipStream_t st = (hipStream_t)stream;
#define PCM_DECODE(F) VIAI_LAUNCH(pcm_decode_kernel<F>, grid, dim3(PCM_THREADS), lds, st, src, channels, frames, mono, out, out_stride)
    PCM_BY_FORMAT(fmt, PCM_DECODE)
#undef PCM_DECODE
    return viai_launch_status();
}

extern "C" long viai_pcm_ws_bytes(long frames) {
    if (frames < 0) return 0;
    const long t = pcm_tiles(frames);
    return 4 * (t < 1 ? 1 : t);
}

extern "C" int viai_pcm_peak(const float* wav, long stride, int channels, long frames, float* ws, void* stream) {
    if (wav == nullptr || ws == nullptr || !pcm_shape_ok(VIAI_PCM_S16, channels, frames) || stride < frames || !pcm_aligned(wav, 4) ||
        !pcm_aligned(ws, 4))
        return (int)hipErrorInvalidValue;
    if (frames == 0) return 0;
    VIAI_LAUNCH(pcm_peak_kernel, dim3((unsigned)pcm_tiles(frames)), dim3(PCM_THREADS), 0, (hipStream_t)stream, wav, stride, channels, frames,
                reinterpret_cast<unsigned*>(ws));
    return viai_launch_status();
}

extern "C" int viai_pcm_encode(const float* wav, long stride, int channels, long frames, int fmt, int normalize, unsigned char* dst, void* ws,
                               void* stream) {
    if (wav == nullptr || dst == nullptr || !pcm_shape_ok(fmt, channels, frames) || stride < frames || !pcm_aligned(wav, 4) ||
        !pcm_aligned(dst, 16) || (normalize && (fmt != VIAI_PCM_S16 || ws == nullptr || !pcm_aligned(ws, 4))))
        return (int)hipErrorInvalidValue;
    if (frames == 0) return 0;
    const long ntiles = pcm_tiles(frames);
    const size_t lds = (size_t)PCM_TILE * channels * pcm_bytes(fmt);
    const dim3 grid((unsigned)(ntiles < PCM_MAX_BLOCKS ? ntiles : PCM_MAX_BLOCKS));
    hipStream_t st = (hipStream_t)stream;
    if (normalize)
        VIAI_LAUNCH(pcm_peak_kernel, dim3((unsigned)ntiles), dim3(PCM_THREADS), 0, st, wav, stride, channels, frames, static_cast<unsigned*>(ws));
#define PCM_ENCODE(F) \
    VIAI_LAUNCH(pcm_encode_kernel<F>, grid, dim3(PCM_THREADS), lds, st, wav, stride, channels, frames, normalize, dst, static_cast<const unsigned*>(ws), ntiles)
    PCM_BY_FORMAT(fmt, PCM_ENCODE)
#undef PCM_ENCODE
    return viai_launch_status();
}

extern "C" int viai_pcm_patch(const float* wav, long stride, int channels, long frames, int fmt, const int* count, const int* start,
                              const int* length, int K, unsigned char* dst, void* stream) {
    if (wav == nullptr || dst == nullptr || count == nullptr || start == nullptr || length == nullptr || !pcm_shape_ok(fmt, channels, frames) ||
        stride < frames || K < 1 || (long)channels * K > 65535 || !pcm_aligned(wav, 4))
        return (int)hipErrorInvalidValue;
    if (frames == 0) return 0;
    const long along = (frames + PCM_THREADS - 1) / PCM_THREADS;
    const dim3 grid((unsigned)(along < PCM_PATCH_BLOCKS ? along : PCM_PATCH_BLOCKS), (unsigned)(channels * K));
    VIAI_LAUNCH(pcm_patch_kernel, grid, dim3(PCM_THREADS), 0, (hipStream_t)stream, wav, stride, channels, frames, fmt, count, start, length, K, dst);
    return viai_launch_status();
}

// ---- the host mirrors: the same rule header, frame by frame, every pointer in host memory
extern "C" int viai_pcm_decode_host(const unsigned char* src, int fmt, int channels, long frames, int mono, float* out, long out_stride) {
    if (src == nullptr || out == nullptr || !pcm_shape_ok(fmt, channels, frames) || out_stride < frames) return (int)hipErrorInvalidValue;
    const int bps = pcm_bytes(fmt);
    for (long i = 0; i < frames; ++i) {
        float acc = 0.f;
        for (int c = 0; c < channels; ++c) {
            const float v = pcm_decode(fmt, pcm_host_get(src + (i * channels + c) * bps, bps));
            if (mono)
                acc = c == 0 ? v : acc + v;
            else
                out[c * out_stride + i] = v;
        }
        if (mono) out[i] = pcm_mono(acc, channels);
    }
    return 0;
}

extern "C" int viai_pcm_encode_host(const float* wav, long stride, int channels, long frames, int fmt, int normalize, unsigned char* dst) {
    if (wav == nullptr || dst == nullptr || !pcm_shape_ok(fmt, channels, frames) || stride < frames || (normalize && fmt != VIAI_PCM_S16))
        return (int)hipErrorInvalidValue;
    const int bps = pcm_bytes(fmt);
    float scale = 0.f;
    if (normalize) {
        float peak = 0.f;
        for (int c = 0; c < channels; ++c)
            for (long i = 0; i < frames; ++i) {
                const float x = wav[c * stride + i], a = x < 0.f ? -x : x;
                if (pcm_finite(x) && a > peak) peak = a;
            }
        scale = pcm_norm_scale(peak);
    }
    for (long i = 0; i < frames; ++i)
        for (int c = 0; c < channels; ++c) {
            const float x = wav[c * stride + i];
            pcm_host_put(dst + (i * channels + c) * bps, bps, normalize ? pcm_encode_norm(x, scale) : pcm_encode(fmt, x));
        }
    return 0;
}

extern "C" int viai_pcm_patch_host(const float* wav, long stride, int channels, long frames, int fmt, const int* count, const int* start,
                                   const int* length, int K, unsigned char* dst) {
    if (wav == nullptr || dst == nullptr || count == nullptr || start == nullptr || length == nullptr || !pcm_shape_ok(fmt, channels, frames) ||
        stride < frames || K < 1 || (long)channels * K > 65535)
        return (int)hipErrorInvalidValue;
    const int bps = pcm_bytes(fmt);
    for (int c = 0; c < channels; ++c)
        for (int k = 0; k < K && k < count[c]; ++k) {
            long s = start[(long)c * K + k], e = s + (long)length[(long)c * K + k];
            s = s < 0 ? 0 : s;
            e = e > frames ? frames : e;
            for (long i = s; i < e; ++i) pcm_host_put(dst + (i * channels + c) * bps, bps, pcm_encode(fmt, wav[c * stride + i]));
        }
    return 0;
}
