// The mixture-of-logistics draw (mixture.py:117-153) shared by viai_mol_sample (wavenet_ops.hip) and the heads of the synthesis chain
// (wavenet.hip): ONE device function, so that a sample drawn step by step is the sample the batched sampler draws from the same row.
#pragma once
#include "viai_common.h"

// y: [logit | mean | log_scale] x K; u1: K uniforms for the Gumbel arg-max over the logits, u2: one for the logistic; all in (1e-5, 1 - 1e-5).
// K is a value: with a compile-time K (mol_sample_kernel<K>) the compiler unrolls the loop in full, with the heads' run-time K it stays a loop.
__device__ __forceinline__ float viai_mol_draw(const float* __restrict__ y, const float* __restrict__ u1, float u2, int K, float log_scale_min) {
    float best = -INFINITY; int arg = 0;
    for (int k = 0; k < K; ++k) {
        const float t = y[k] - logf(-logf(u1[k]));
        if (t > best) { best = t; arg = k; }
    }
    const float m = y[K + arg], ls = fmaxf(y[2 * K + arg], log_scale_min);
    const float x = m + expf(ls) * (logf(u2) - logf(1.f - u2));
    return fminf(fmaxf(x, -1.f), 1.f);
}
