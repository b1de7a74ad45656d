// mu-law companding shared by viai_mulaw_quantize (wavenet_ops.hip) and the utterance preparation (preprocess.hip): ONE pair of device functions,
// so that a class computed on the fly while trimming is the class viai_mulaw_quantize writes for the same float (utils/librivox.py:66-74).
#pragma once
#include "viai_common.h"

// y = sign(x) log1p(mu |x|) / log1p(mu); l1p = log1pf(mu).  A division: |x| = 1 gives exactly 1, class mu.
__device__ __forceinline__ float viai_mulaw_compand(float xx, float mu, float l1p) {
    const float mag = log1pf(mu * fabsf(xx)) / l1p;
    return xx < 0.f ? -mag : mag;
}

// class = trunc((y + 1) / 2 * mu) clamped to [0, mu]
__device__ __forceinline__ int viai_mulaw_class_of(float y, float mu) {
    const int k = (int)((y + 1.f) * 0.5f * mu);                  // truncation
    return min(max(k, 0), (int)mu);
}

__device__ __forceinline__ int viai_mulaw_class(float xx, float mu, float l1p) { return viai_mulaw_class_of(viai_mulaw_compand(xx, mu, l1p), mu); }
