// Waveform inpainting around the WaveNet synthesis loop (gfx950): cut per-stream windows [receptive field | gap] out of a clip and its up-sampled
// conditioning, and put the generated samples back.  The loop itself is the synthesis chain of csrc/wavenet.hip with a mask of forced steps
// (viai_wavenet_synth_run_forced): the R samples in front of a gap are teacher-forced (they fill the dilated convs' ring buffers the way
// wavenet.py:322-327 does with test_inputs), the gap runs free.  Window arithmetic: include/viai_hip.h, DESIGN.md 11.2f.
#include "viai_common.h"
#include "viai_internal.h"

namespace {

// item i = (row r = b L + t, column group c of q): the conditioning row's float4 number c; the item with c == 0 also writes the row's input
// and its mask entry.  Source time s = w[b] + t; outside [0, n) the clip is silent (0.0 / `silence` / a zero conditioning row).
__global__ __launch_bounds__(256) void wn_window_gather_kernel(const float* __restrict__ wav, const int* __restrict__ classes, const float* __restrict__ cond,
                                                               const int* __restrict__ w, const int* __restrict__ len, float* __restrict__ x_out,
                                                               int* __restrict__ cls_out, float* __restrict__ cond_out, unsigned char* __restrict__ forced,
                                                               int B, int n, int L, int R, int cin, int q, int silence) {
    const long total = (long)B * L * q;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256L) {
        const long r = i / q;
        const int c = (int)(i - r * q);
        const int b = (int)(r / L), t = (int)(r - (long)b * L);
        const long s = (long)w[b] + t;
        const bool inside = s >= 0 && s < n;
        const size_t src = (size_t)b * n + (size_t)(inside ? s : 0);
        if (cond != nullptr) {
            f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
            if (inside) v = *reinterpret_cast<const f32x4*>(cond + src * cin + 4 * c);
            *reinterpret_cast<f32x4*>(cond_out + (size_t)r * cin + 4 * c) = v;
        }
        if (c == 0) {
            if (wav != nullptr) x_out[r] = inside ? wav[src] : 0.f;
            if (classes != nullptr) cls_out[r] = inside ? classes[src] : silence;
            const int k = t - R;
            forced[r] = (k >= 0 && k < len[b]) ? 0 : 1;
        }
    }
}

// out = wav outside [g0, g0 + len); inside, the generated sample of window position R + (i - g0), blended into the original over the gap's last
// `fade` samples.  Products and sums are rounded one by one (no fused multiply-add), so the blend is the fp32 formula of the header bit for bit.
__global__ __launch_bounds__(256) void wn_splice_kernel(const float* __restrict__ wav, const float* __restrict__ gen, const int* __restrict__ g0,
                                                        const int* __restrict__ len, float* __restrict__ out, int B, int n, int L, int R, int fade) {
    const long total = (long)B * n;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256L) {
        const int b = (int)(i / n), s = (int)(i - (long)b * n);
        const float o = wav[i];
        float v = o;
        const long k = (long)s - g0[b];                              // position inside the gap
        const int ln = len[b];
        if (k >= 0 && k < ln && R + k < L) {
            const float g = gen[(size_t)b * L + R + k];
            v = g;
            const long j = k - ((long)ln - fade);                    // position inside the fade
            if (fade > 0 && j >= 0) {
                const float a = __fdiv_rn((float)(j + 1), (float)(fade + 1));
                v = __fadd_rn(g, __fmul_rn(a, __fsub_rn(o, g)));
            }
        }
        out[i] = v;
    }
}

}  // namespace

extern "C" int viai_wn_window_gather(const float* wav, const int* classes, const float* cond, const int* w, const int* len, float* x_out, int* cls_out,
                                     float* cond_out, unsigned char* forced, int B, int n, int L, int R, int cin, int silence_class, void* stream) {
    if (B < 1 || n < 1 || L < 1 || R < 0 || w == nullptr || len == nullptr || forced == nullptr) return (int)hipErrorInvalidValue;
    if ((wav == nullptr && classes == nullptr) || (wav != nullptr && x_out == nullptr) || (classes != nullptr && cls_out == nullptr))
        return (int)hipErrorInvalidValue;
    if (cond != nullptr && (cond_out == nullptr || cin < 4 || cin % 4 != 0)) return (int)hipErrorInvalidValue;
    const int q = cond != nullptr ? cin / 4 : 1;
    VIAI_LAUNCH(wn_window_gather_kernel, dim3(viai_ew_blocks((long)B * L * q)), dim3(256), 0, (hipStream_t)stream, wav, classes, cond, w, len, x_out, cls_out,
                cond_out, forced, B, n, L, R, cin, q, silence_class);
    return viai_launch_status();
}

extern "C" int viai_wn_splice(const float* wav, const float* gen, const int* g0, const int* len, float* out, int B, int n, int L, int R, int fade,
                              void* stream) {
    if (B < 1 || n < 1 || L < 1 || R < 0 || fade < 0 || wav == nullptr || gen == nullptr || g0 == nullptr || len == nullptr || out == nullptr)
        return (int)hipErrorInvalidValue;
    VIAI_LAUNCH(wn_splice_kernel, dim3(viai_ew_blocks((long)B * n)), dim3(256), 0, (hipStream_t)stream, wav, gen, g0, len, out, B, n, L, R, fade);
    return viai_launch_status();
}
