// WaveNet vocoder pieces that are not convolutions (gfx950): weight normalisation, the gated activation,
// residual / skip scaling, the scalar-input first layer, the conditioning up-sampler, the discretised
// mixture-of-logistics loss and sampler.  The dilated / 1x1 Conv1d layers themselves run on the implicit-GEMM
// MFMA kernels (conv_igemm.hip, H = 1).  Reference: wavenet_vocoder/{wavenet,modules,mixture}.py.
// Activations are (B, 1, T, C) NHWC, i.e. (B*T) rows of C channels.
#include "viai_common.h"
#include "viai_internal.h"
#include "viai_mulaw.h"

namespace {

inline int ew_blocks(long n) {
    long b = (n + 255) / 256;
    if (b > 8192) b = 8192;
    if (b < 1) b = 1;
    return (int)b;
}

__device__ __forceinline__ float block_sum(float v, float* red) {      // 256 threads
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// ---------------------------------------------------------------- weight norm (modules.py:39, torch weight_norm dim=0)
// w[r][:] = g[r] * v[r][:] / ||v[r]||      one block per row r
__global__ __launch_bounds__(256) void weight_norm_fwd_kernel(const float* __restrict__ v, const float* __restrict__ g,
                                                              float* __restrict__ w, float* __restrict__ norm, int L) {
    __shared__ float red[4];
    const int r = blockIdx.x;
    float s = 0.f;
    for (int i = threadIdx.x; i < L; i += 256) { float t = v[(size_t)r * L + i]; s += t * t; }
    const float n = sqrtf(block_sum(s, red));
    const float sc = g[r] / n;
    for (int i = threadIdx.x; i < L; i += 256) w[(size_t)r * L + i] = v[(size_t)r * L + i] * sc;
    if (threadIdx.x == 0) norm[r] = n;
}

// dg[r] = <dw, v>/n ;  dv = g/n * (dw - v * <dw, v>/n^2)
__global__ __launch_bounds__(256) void weight_norm_bwd_kernel(const float* __restrict__ dw, const float* __restrict__ v,
                                                              const float* __restrict__ g, const float* __restrict__ norm,
                                                              float* __restrict__ dv, float* __restrict__ dg, int L, int accumulate) {
    __shared__ float red[4];
    const int r = blockIdx.x;
    float s = 0.f;
    for (int i = threadIdx.x; i < L; i += 256) s += dw[(size_t)r * L + i] * v[(size_t)r * L + i];
    const float dot = block_sum(s, red);
    const float n = norm[r], gs = g[r] / n, k = dot / (n * n);
    for (int i = threadIdx.x; i < L; i += 256) {
        float t = gs * (dw[(size_t)r * L + i] - v[(size_t)r * L + i] * k);
        dv[(size_t)r * L + i] = accumulate ? dv[(size_t)r * L + i] + t : t;
    }
    if (threadIdx.x == 0) dg[r] = accumulate ? dg[r] + dot / n : dot / n;
}

// ---------------------------------------------------------------- gated activation (modules.py:183-201)
// y, yc: rows of 2*H channels [a | b];  z[row][h] = tanh(a + ca) * sigmoid(b + cb)
__global__ __launch_bounds__(256) void glu_fwd_kernel(const float* __restrict__ y, const float* __restrict__ yc,
                                                      float* __restrict__ z, long rows, int H) {
    const int h4n = H / 4;
    const long total = rows * h4n;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256L) {
        long r = i / h4n; int h = (int)(i % h4n) * 4;
        f32x4 a = *reinterpret_cast<const f32x4*>(y + r * 2 * H + h), b = *reinterpret_cast<const f32x4*>(y + r * 2 * H + H + h);
        if (yc) { a += *reinterpret_cast<const f32x4*>(yc + r * 2 * H + h); b += *reinterpret_cast<const f32x4*>(yc + r * 2 * H + H + h); }
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = tanhf(a[e]) * (1.f / (1.f + expf(-b[e])));
        *reinterpret_cast<f32x4*>(z + r * H + h) = o;
    }
}

// dy[row] = [dz*(1-tanh^2)*sig | dz*tanh*sig*(1-sig)]   (the same tensor is the gradient of y AND of yc)
__global__ __launch_bounds__(256) void glu_bwd_kernel(const float* __restrict__ dz, const float* __restrict__ y, const float* __restrict__ yc,
                                                      float* __restrict__ dy, long rows, int H) {
    const int h4n = H / 4;
    const long total = rows * h4n;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256L) {
        long r = i / h4n; int h = (int)(i % h4n) * 4;
        f32x4 a = *reinterpret_cast<const f32x4*>(y + r * 2 * H + h), b = *reinterpret_cast<const f32x4*>(y + r * 2 * H + H + h);
        if (yc) { a += *reinterpret_cast<const f32x4*>(yc + r * 2 * H + h); b += *reinterpret_cast<const f32x4*>(yc + r * 2 * H + H + h); }
        f32x4 g = *reinterpret_cast<const f32x4*>(dz + r * H + h), da, db;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float t = tanhf(a[e]), s = 1.f / (1.f + expf(-b[e]));
            da[e] = g[e] * (1.f - t * t) * s;
            db[e] = g[e] * t * s * (1.f - s);
        }
        *reinterpret_cast<f32x4*>(dy + r * 2 * H + h) = da;
        *reinterpret_cast<f32x4*>(dy + r * 2 * H + H + h) = db;
    }
}

// out = (a + b) * s   (b may be null: out = a * s)
__global__ __launch_bounds__(256) void add_scale_kernel(const f32x4* __restrict__ a, const f32x4* __restrict__ b, f32x4* __restrict__ o, float s, long n4) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n4; i += (long)gridDim.x * 256L) o[i] = b ? (a[i] + b[i]) * s : a[i] * s;
}

__global__ __launch_bounds__(256) void relu_fwd_kernel(const f32x4* __restrict__ a, f32x4* __restrict__ o, long n4) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n4; i += (long)gridDim.x * 256L) {
        f32x4 v = a[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : 0.f;
        o[i] = v;
    }
}

// ---------------------------------------------------------------- scalar-input first conv (wavenet.py:118: Conv1d1x1(1, C))
// y[p][c] = x[p] * w[c] + b[c]
__global__ __launch_bounds__(256) void outer_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                                                        float* __restrict__ y, long rows, int C) {
    const int c4n = C / 4;
    const long total = rows * c4n;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256L) {
        long r = i / c4n; int c = (int)(i % c4n) * 4;
        f32x4 wv = *reinterpret_cast<const f32x4*>(w + c), bv = *reinterpret_cast<const f32x4*>(b + c);
        *reinterpret_cast<f32x4*>(y + r * C + c) = x[r] * wv + bv;
    }
}

// part[blk][0][c] = sum_p dy[p][c] * x[p];  part[blk][1][c] = sum_p dy[p][c]
__global__ __launch_bounds__(256) void outer_bwd_part_kernel(const float* __restrict__ dy, const float* __restrict__ x, float* __restrict__ part,
                                                             long rows, int C, long rows_per_blk) {
    __shared__ f32x4 r1[256], r2[256];
    const int tid = threadIdx.x, CG = C / 4;
    const long row0 = blockIdx.x * rows_per_blk;
    long row1 = row0 + rows_per_blk; if (row1 > rows) row1 = rows;
    for (int g0 = 0; g0 < CG; g0 += 256) {
        const int cgw = min(256, CG - g0), pg = 256 / cgw, cg = tid % cgw, pl = tid / cgw;
        f32x4 s1 = {0.f, 0.f, 0.f, 0.f}, s2 = {0.f, 0.f, 0.f, 0.f};
        // rows in runs of 32 per lane, each run summed on its own: a lane's fp32 error stays that of two short sums (C > 1024 leaves one lane
        // per column group, up to 1024 rows in a single accumulator: 4.8 x the error of torch's fp32 column sum at 1000 rows)
        if (pl < pg)
            for (long r = row0 + pl; r < row1;) {
                f32x4 p1 = {0.f, 0.f, 0.f, 0.f}, p2 = {0.f, 0.f, 0.f, 0.f};
                for (int u = 0; u < 32 && r < row1; ++u, r += pg) {
                    f32x4 g = *reinterpret_cast<const f32x4*>(dy + r * C + (g0 + cg) * 4);
                    p1 += g * x[r]; p2 += g;
                }
                s1 += p1; s2 += p2;
            }
        r1[tid] = s1; r2[tid] = s2;
        __syncthreads();
        if (tid < cgw) {
            f32x4 t1 = {0.f, 0.f, 0.f, 0.f}, t2 = {0.f, 0.f, 0.f, 0.f};
            for (int k = 0; k < pg; ++k) { t1 += r1[k * cgw + tid]; t2 += r2[k * cgw + tid]; }
            *reinterpret_cast<f32x4*>(part + ((size_t)blockIdx.x * 2 + 0) * C + (g0 + tid) * 4) = t1;
            *reinterpret_cast<f32x4*>(part + ((size_t)blockIdx.x * 2 + 1) * C + (g0 + tid) * 4) = t2;
        }
        __syncthreads();
    }
}

__global__ void outer_bwd_final_kernel(const float* __restrict__ part, int nblk, int C, float* dw, float* db, int accumulate) {
    int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double s1 = 0.0, s2 = 0.0;
    for (int b = 0; b < nblk; ++b) { s1 += (double)part[((size_t)b * 2) * C + c]; s2 += (double)part[((size_t)b * 2 + 1) * C + c]; }
    dw[c] = accumulate ? dw[c] + (float)s1 : (float)s1;
    db[c] = accumulate ? db[c] + (float)s2 : (float)s2;
}

// ---------------------------------------------------------------- conditioning up-sampler (wavenet.py:153-164)
// ConvTranspose2d(1, 1, (KH, S), stride (1, S), padding ((KH-1)/2, 0)) + ReLU on (B, F, T):
//   out[b][f][t*S + j] = relu(bias + sum_r in[b][f + P - r][t] * w[r][j])
template <int KH>
__global__ __launch_bounds__(256) void upsample_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                           float* __restrict__ y, long BF, int F, int T, int S) {
    constexpr int P = (KH - 1) / 2;
    const long total = BF * T * S;
    const float b0 = bias[0];
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256L) {
        long bf = i / ((long)T * S); int to = (int)(i % ((long)T * S));
        int t = to / S, j = to % S, f = (int)(bf % F);
        float acc = b0;
#pragma unroll
        for (int r = 0; r < KH; ++r) {
            int fi = f + P - r;
            if ((unsigned)fi < (unsigned)F) acc += x[(bf - f + fi) * T + t] * w[r * S + j];
        }
        y[i] = acc > 0.f ? acc : 0.f;
    }
}

// dx[b][f][t] = sum_{r,j} dpre[b][f - P + r][t*S + j] * w[r][j],  dpre = dy * (y > 0)
template <int KH>
__global__ __launch_bounds__(256) void upsample_bwd_x_kernel(const float* __restrict__ dy, const float* __restrict__ y, const float* __restrict__ w,
                                                             float* __restrict__ dx, long BF, int F, int T, int S) {
    constexpr int P = (KH - 1) / 2;
    const long total = BF * T;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256L) {
        long bf = i / T; int t = (int)(i % T), f = (int)(bf % F);
        float acc = 0.f;
#pragma unroll
        for (int r = 0; r < KH; ++r) {
            int fo = f - P + r;
            if ((unsigned)fo >= (unsigned)F) continue;
            const long base = ((bf - f + fo) * T + t) * S;
            for (int j = 0; j < S; ++j) { float g = y[base + j] > 0.f ? dy[base + j] : 0.f; acc += g * w[r * S + j]; }
        }
        dx[i] = acc;
    }
}

// part[blk][r*S + j] = sum dpre[b][f][t*S+j] * x[b][f + P - r][t];  part[blk][KH*S] = sum dpre     (S <= 16)
template <int KH>
__global__ __launch_bounds__(256) void upsample_bwd_w_kernel(const float* __restrict__ dy, const float* __restrict__ y, const float* __restrict__ x,
                                                             float* __restrict__ part, long BF, int F, int T, int S) {
    constexpr int P = (KH - 1) / 2;
    __shared__ float red[4];
    float acc[KH * 16 + 1];
#pragma unroll
    for (int k = 0; k < KH * 16 + 1; ++k) acc[k] = 0.f;
    const long total = BF * T;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256L) {
        long bf = i / T; int t = (int)(i % T), f = (int)(bf % F);
        float xin[KH];
#pragma unroll
        for (int r = 0; r < KH; ++r) { int fi = f + P - r; xin[r] = ((unsigned)fi < (unsigned)F) ? x[(bf - f + fi) * T + t] : 0.f; }
        const long base = (bf * T + t) * S;
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (j < S) {
                float g = y[base + j] > 0.f ? dy[base + j] : 0.f;
                acc[KH * 16] += g;
#pragma unroll
                for (int r = 0; r < KH; ++r) acc[r * 16 + j] += g * xin[r];
            }
    }
    for (int k = 0; k < KH * 16 + 1; ++k) {
        float s = block_sum(acc[k], red);
        if (threadIdx.x == 0) part[(size_t)blockIdx.x * (KH * 16 + 1) + k] = s;
    }
}

__global__ void upsample_bwd_final_kernel(const float* __restrict__ part, int nblk, int KH, int S, float* dw, float* db, int accumulate) {
    int k = threadIdx.x;
    const int W = KH * 16 + 1;
    if (k >= W) return;
    double s = 0.0;
    for (int b = 0; b < nblk; ++b) s += (double)part[(size_t)b * W + k];
    if (k == KH * 16) { db[0] = accumulate ? db[0] + (float)s : (float)s; return; }
    int r = k / 16, j = k % 16;
    if (j < S) dw[r * S + j] = accumulate ? dw[r * S + j] + (float)s : (float)s;
}

// ---------------------------------------------------------------- discretised mixture of logistics (mixture.py:25-105)
__device__ __forceinline__ float softplusf(float x) { return x > 20.f ? x : log1pf(expf(x)); }   // torch softplus (threshold 20)
__device__ __forceinline__ float sigmoidf(float x) { return 1.f / (1.f + expf(-x)); }

// yhat: rows of `pitch` floats, first 3*K are [logit | mean | log_scale]; target y[row]; out loss[row] = -logsumexp_k(...)
// dyh (optional, same pitch): d(sum_rows wrow[row] * loss[row]) / d yhat
template <int K>
__global__ __launch_bounds__(256) void mol_loss_kernel(const float* __restrict__ yhat, const float* __restrict__ y, const float* __restrict__ wrow,
                                                       float* __restrict__ loss, float* __restrict__ dyh, long rows, int pitch,
                                                       float num_classes, float log_scale_min) {
    const float h = 1.f / (num_classes - 1.f), logh2 = logf((num_classes - 1.f) * 0.5f);
    for (long r = blockIdx.x * 256L + threadIdx.x; r < rows; r += (long)gridDim.x * 256L) {
        const float* p = yhat + r * pitch;
        const float yy = y[r];
        float logit[K], lp[K], dm[K], dls[K];
        float mx = -INFINITY;
#pragma unroll
        for (int k = 0; k < K; ++k) { logit[k] = p[k]; mx = fmaxf(mx, logit[k]); }
        float se = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) se += expf(logit[k] - mx);
        const float lse_logit = mx + logf(se);
        float best = -INFINITY;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const float m = p[K + k], lsr = p[2 * K + k];
            const bool clamped = lsr < log_scale_min;
            const float ls = clamped ? log_scale_min : lsr;
            const float inv = expf(-ls), c = yy - m;
            const float pin = inv * (c + h), min_ = inv * (c - h), mid = inv * c;
            float v, gm, gs;                              // value, d/dmean, d/dlog_scale
            if (yy < -0.999f) {
                v = pin - softplusf(pin);
                float d = sigmoidf(-pin);
                gm = d * (-inv); gs = d * (-pin);
            } else if (yy > 0.999f) {
                v = -softplusf(min_);
                float d = -sigmoidf(min_);
                gm = d * (-inv); gs = d * (-min_);
            } else {
                const float sp = sigmoidf(pin), sm = sigmoidf(min_), cd = sp - sm;
                if (cd > 1e-5f) {
                    v = logf(fmaxf(cd, 1e-12f));
                    const float dp = sp * (1.f - sp) / cd, dn = -sm * (1.f - sm) / cd;
                    gm = (dp + dn) * (-inv); gs = dp * (-pin) + dn * (-min_);
                } else {
                    v = mid - ls - 2.f * softplusf(mid) - logh2;
                    const float d = 1.f - 2.f * sigmoidf(mid);
                    gm = d * (-inv); gs = d * (-mid) - 1.f;
                }
            }
            if (clamped) gs = 0.f;
            lp[k] = v + (logit[k] - lse_logit);
            dm[k] = gm; dls[k] = gs;
            best = fmaxf(best, lp[k]);
        }
        float s2 = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) s2 += expf(lp[k] - best);
        const float lse = best + logf(s2);
        loss[r] = -lse;
        if (dyh) {
            const float wr = wrow ? wrow[r] : 1.f;
            float* q = dyh + r * pitch;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const float pk = expf(lp[k] - lse);                 // posterior responsibility
                const float sk = expf(logit[k] - lse_logit);        // prior softmax
                q[k] = wr * (sk - pk);
                q[K + k] = wr * (-pk * dm[k]);
                q[2 * K + k] = wr * (-pk * dls[k]);
            }
            for (int k = 3 * K; k < pitch; ++k) q[k] = 0.f;
        }
    }
}

// sample (mixture.py:117-153) with INJECTED uniforms u1[row][K], u2[row] in (1e-5, 1-1e-5)
template <int K>
__global__ __launch_bounds__(256) void mol_sample_kernel(const float* __restrict__ yhat, const float* __restrict__ u1, const float* __restrict__ u2,
                                                         float* __restrict__ out, long rows, int pitch, float log_scale_min) {
    for (long r = blockIdx.x * 256L + threadIdx.x; r < rows; r += (long)gridDim.x * 256L) {
        const float* p = yhat + r * pitch;
        float best = -INFINITY; int arg = 0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            float t = p[k] - logf(-logf(u1[r * K + k]));
            if (t > best) { best = t; arg = k; }
        }
        const float m = p[K + arg], ls = fmaxf(p[2 * K + arg], log_scale_min), u = u2[r];
        float x = m + expf(ls) * (logf(u) - logf(1.f - u));
        out[r] = fminf(fmaxf(x, -1.f), 1.f);
    }
}

// masked mean: out = sum(loss * mask) / sum(mask)     (loss_functions.py:43-62)
__global__ __launch_bounds__(256) void masked_mean_kernel(const float* __restrict__ loss, const float* __restrict__ mask, long n, float* out, float* wrow) {
    __shared__ double r1[4], r2[4];
    double a = 0.0, b = 0.0;
    for (long i = threadIdx.x; i < n; i += 256) { float m = mask ? mask[i] : 1.f; a += (double)loss[i] * m; b += m; }
    a = wave_sum_d(a); b = wave_sum_d(b);
    if ((threadIdx.x & 63) == 0) { r1[threadIdx.x >> 6] = a; r2[threadIdx.x >> 6] = b; }
    __syncthreads();
    const double sa = r1[0] + r1[1] + r1[2] + r1[3], sb = r2[0] + r2[1] + r2[2] + r2[3];
    if (threadIdx.x == 0) *out = (float)(sa / sb);
    if (wrow) for (long i = threadIdx.x; i < n; i += 256) wrow[i] = (mask ? mask[i] : 1.f) / (float)sb;
}

// ---------------------------------------------------------------- masked cross entropy on NHWC rows (loss_functions.py:24-40)
// One wave per row; lane l holds the float4 column groups 4 l + 256 j (j < NV) of its row, so K = 256 is one 16-byte load per lane.
constexpr int CE_MAXV = 4;                                            // K <= 1024

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// the row's columns into registers (-inf beyond K), its maximum and sum of exp(x - max): the same instructions in both passes, so the
// softmax of pass 2 is built from the bits pass 1 saw
template <int NV>
__device__ __forceinline__ void ce_row_load(const float* __restrict__ p, int K, int lane, f32x4 (&v)[NV], float& mx, float& se) {
    mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int c = 4 * lane + 256 * j;
        if (c < K) v[j] = *reinterpret_cast<const f32x4*>(p + c);
        else v[j] = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        mx = fmaxf(mx, fmaxf(fmaxf(v[j][0], v[j][1]), fmaxf(v[j][2], v[j][3])));
    }
    mx = wave_max(mx);
    se = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) se += expf(v[j][e] - mx);        // exp(-inf) = 0 in the columns beyond K
    se = wave_sum(se);
}

// row (b, t) is scored against target (b, t + shift); tgt < 0 means "no target" (the last `shift` rows of a stream)
__device__ __forceinline__ void ce_row_target(const int* __restrict__ target, const float* __restrict__ mask, long r, int T, int shift,
                                              int& tgt, float& m) {
    const long b = r / T;
    const int t = (int)(r - b * T);
    if (t + shift < T) {
        tgt = target[r + shift];
        m = mask ? mask[b * (T - shift) + t] : 1.f;
    } else {
        tgt = -1;
        m = 0.f;
    }
}

// pass 1: loss[row] = logsumexp(row) - row[target]; meff[row] = the mask as applied (0 on the rows without a target)
template <int NV>
__global__ __launch_bounds__(256) void masked_ce_rows_kernel(const float* __restrict__ logits, const int* __restrict__ target,
                                                             const float* __restrict__ mask, float* __restrict__ loss, float* __restrict__ meff,
                                                             long rows, int T, int K, int pitch, int shift) {
    const int lane = threadIdx.x & 63;
    for (long r = blockIdx.x * 4L + (threadIdx.x >> 6); r < rows; r += gridDim.x * 4L) {
        int tgt; float m;
        ce_row_target(target, mask, r, T, shift, tgt, m);
        f32x4 v[NV];
        float mx, se;
        ce_row_load<NV>(logits + r * pitch, K, lane, v, mx, se);
        float xt = 0.f;                                              // the target's logit less the maximum, picked by column number
#pragma unroll
        for (int j = 0; j < NV; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) xt += (4 * lane + 256 * j + e == tgt) ? v[j][e] - mx : 0.f;
        xt = wave_sum(xt);                                           // one non-zero addend at most: exact
        if (lane == 0) {
            const bool in_range = tgt >= 0 && tgt < K;
            // log(se) - (x_t - max), not (max + log(se)) - x_t: the maximum never meets the small term, so rows of large logits keep its bits
            loss[r] = in_range ? logf(se) - xt : (m != 0.f ? NAN : 0.f);
            meff[r] = m;
        }
    }
}

// pass 2: dlogits[row][c] = wrow[row] * (softmax(row)[c] - [c == target]); zeros in the columns K .. pitch and on the rows of weight 0
template <int NV>
__global__ __launch_bounds__(256) void masked_ce_grad_kernel(const float* __restrict__ logits, const int* __restrict__ target,
                                                             const float* __restrict__ wrow, float* __restrict__ dlogits,
                                                             long rows, int T, int K, int pitch, int shift) {
    const int lane = threadIdx.x & 63;
    for (long r = blockIdx.x * 4L + (threadIdx.x >> 6); r < rows; r += gridDim.x * 4L) {
        const long b = r / T;
        const int t = (int)(r - b * T);
        const float w = wrow[r];
        const int tgt = t + shift < T ? target[r + shift] : -1;
        float* q = dlogits + r * pitch;
        const f32x4 zero = f32x4{0.f, 0.f, 0.f, 0.f};
        if (w == 0.f) {                                              // wave-uniform
            for (int c = 4 * lane; c < pitch; c += 256) *reinterpret_cast<f32x4*>(q + c) = zero;
            continue;
        }
        f32x4 v[NV];
        float mx, se;
        ce_row_load<NV>(logits + r * pitch, K, lane, v, mx, se);
        const float lg = logf(se);
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int c = 4 * lane + 256 * j;
            if (c < K) {
                f32x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = w * (expf((v[j][e] - mx) - lg) - (c + e == tgt ? 1.f : 0.f));
                *reinterpret_cast<f32x4*>(q + c) = o;
            } else if (c < pitch) {
                *reinterpret_cast<f32x4*>(q + c) = zero;
            }
        }
        for (int c = 4 * lane + 256 * NV; c < pitch; c += 256) *reinterpret_cast<f32x4*>(q + c) = zero;
    }
}

// ---------------------------------------------------------------- first_conv on class indices (wavenet.py:118 on one-hot rows)
// wt[k][c] = w[c][k]: 32 x 32 tiles through LDS, both sides coalesced
__global__ __launch_bounds__(256) void transpose_kernel(const float* __restrict__ w, float* __restrict__ wt, int R, int Cc) {   // w [R][Cc] -> wt [Cc][R]
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
    for (int i = ty; i < 32; i += 8)
        if (r0 + i < R && c0 + tx < Cc) tile[i][tx] = w[(size_t)(r0 + i) * Cc + c0 + tx];
    __syncthreads();
    for (int i = ty; i < 32; i += 8)
        if (c0 + i < Cc && r0 + tx < R) wt[(size_t)(c0 + i) * R + r0 + tx] = tile[tx][i];
}

// h[p][:] = wt[classes[p]][:] + b
__global__ __launch_bounds__(256) void class_embed_fwd_kernel(const int* __restrict__ classes, const f32x4* __restrict__ wt, const f32x4* __restrict__ b,
                                                              f32x4* __restrict__ h, long rows, int K, int C4) {
    const long n = rows * C4;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256L) {
        const long p = i / C4;
        const int c = (int)(i - p * C4);
        const int k = classes[p];
        f32x4 o = f32x4{NAN, NAN, NAN, NAN};
        if (k >= 0 && k < K) o = wt[(size_t)k * C4 + c] + b[c];
        h[i] = o;
    }
}

// Weight gradient of that layer.  Block (k, s) owns class k in the row segment s: its four waves each scan a quarter of a 2048-row chunk of the
// class array and list the rows of class k in LDS (ascending inside a wave's quarter, quarters in order), then thread c4 sums the float4 column
// group c4 of the listed rows of dh in list order, four rows in flight.  part[s][k][:] receives the sum; class_embed_final_kernel adds the
// segments in order.  Every addition has a fixed place: the same bits on every run, no atomics.  dh is read once in total.
constexpr int CEB_CHUNK = 2048;

__global__ __launch_bounds__(256) void class_embed_bwd_part_kernel(const float* __restrict__ dh, const int* __restrict__ classes, float* __restrict__ part,
                                                                   long rows, long seg, int K, int C) {
    __shared__ int list[4][CEB_CHUNK / 4];
    __shared__ int cnt[4];
    const int k = blockIdx.x, s = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int C4 = C / 4;
    const bool own = (int)threadIdx.x < C4;
    const long r_end = (s + 1) * seg < rows ? (s + 1) * seg : rows;
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    for (long base = s * seg; base < r_end; base += CEB_CHUNK) {
        int n = 0;                                                   // wave-uniform
        const long q0 = base + wave * (CEB_CHUNK / 4);
        for (int i = 0; i < CEB_CHUNK / 4; i += 64) {
            const long r = q0 + i + lane;
            const bool hit = r < r_end && classes[r] == k;
            const unsigned long long bal = __ballot(hit);
            if (hit) list[wave][n + __popcll(bal & ((1ull << lane) - 1ull))] = (int)(r - base);
            n += __popcll(bal);
        }
        if (lane == 0) cnt[wave] = n;
        __syncthreads();
        if (own) {
            for (int w = 0; w < 4; ++w) {
                const int nw = cnt[w];
                for (int i = 0; i < nw; i += 4) {
                    f32x4 x[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        if (i + u < nw) x[u] = *reinterpret_cast<const f32x4*>(dh + (size_t)(base + list[w][i + u]) * C + 4 * threadIdx.x);
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        if (i + u < nw) acc += x[u];
                }
            }
        }
        __syncthreads();
    }
    if (own) *reinterpret_cast<f32x4*>(part + ((size_t)s * K + k) * C + 4 * threadIdx.x) = acc;
}

// dw[c][k] = sum_s part[s][k][c] (s ascending): 32 x 32 tiles through LDS into the parameter's [C][K] layout
__global__ __launch_bounds__(256) void class_embed_final_kernel(const float* __restrict__ part, float* __restrict__ dw, int S, int K, int C) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int k0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
    for (int i = ty; i < 32; i += 8) {
        float a = 0.f;
        if (k0 + i < K && c0 + tx < C)
            for (int s = 0; s < S; ++s) a += part[((size_t)s * K + k0 + i) * C + c0 + tx];
        tile[i][tx] = a;
    }
    __syncthreads();
    for (int i = ty; i < 32; i += 8)
        if (c0 + i < C && k0 + tx < K) dw[(size_t)(c0 + i) * K + k0 + tx] = tile[tx][i];
}

// db[c] = sum_k dw[c][k]: one block per channel
__global__ __launch_bounds__(256) void class_embed_bias_kernel(const float* __restrict__ dw, float* __restrict__ db, int K) {
    __shared__ float red[4];
    float a = 0.f;
    for (int k = threadIdx.x; k < K; k += 256) a += dw[(size_t)blockIdx.x * K + k];
    a = block_sum(a, red);
    if (threadIdx.x == 0) db[blockIdx.x] = a;
}

// waveform -> mu-law class (utils/librivox.py:66-74)
__global__ __launch_bounds__(256) void mulaw_quantize_kernel(const float* __restrict__ x, int* __restrict__ cls, long n, float mu) {
    const float l1p = log1pf(mu);
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256L) cls[i] = viai_mulaw_class(x[i], mu, l1p);   // viai_mulaw.h
}

__global__ __launch_bounds__(256) void scale_rows_kernel(float* __restrict__ d, const float* __restrict__ gscale, long n) {
    const float g = *gscale;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256L) d[i] *= g;
}

}  // namespace

extern "C" int viai_weight_norm_fwd(const float* v, const float* g, float* w, float* norm, int rows, int L, void* stream) {
    VIAI_LAUNCH(weight_norm_fwd_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, v, g, w, norm, L);
    return viai_launch_status();
}

extern "C" int viai_weight_norm_bwd(const float* dw, const float* v, const float* g, const float* norm, float* dv, float* dg,
                                    int rows, int L, int accumulate, void* stream) {
    VIAI_LAUNCH(weight_norm_bwd_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, dw, v, g, norm, dv, dg, L, accumulate);
    return viai_launch_status();
}

extern "C" int viai_glu_fwd(const float* y, const float* yc, float* z, long rows, int H, void* stream) {
    if (H % 4 != 0) return (int)hipErrorInvalidValue;
    VIAI_LAUNCH(glu_fwd_kernel, dim3(ew_blocks(rows * (H / 4))), dim3(256), 0, (hipStream_t)stream, y, yc, z, rows, H);
    return viai_launch_status();
}

extern "C" int viai_glu_bwd(const float* dz, const float* y, const float* yc, float* dy, long rows, int H, void* stream) {
    if (H % 4 != 0) return (int)hipErrorInvalidValue;
    VIAI_LAUNCH(glu_bwd_kernel, dim3(ew_blocks(rows * (H / 4))), dim3(256), 0, (hipStream_t)stream, dz, y, yc, dy, rows, H);
    return viai_launch_status();
}

extern "C" int viai_add_scale(const float* a, const float* b, float* out, float s, long n, void* stream) {
    if (n % 4 != 0) return (int)hipErrorInvalidValue;
    VIAI_LAUNCH(add_scale_kernel, dim3(ew_blocks(n / 4)), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const f32x4*>(a),
                reinterpret_cast<const f32x4*>(b), reinterpret_cast<f32x4*>(out), s, n / 4);
    return viai_launch_status();
}

extern "C" int viai_relu_fwd(const float* a, float* out, long n, void* stream) {
    if (n % 4 != 0) return (int)hipErrorInvalidValue;
    VIAI_LAUNCH(relu_fwd_kernel, dim3(ew_blocks(n / 4)), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const f32x4*>(a), reinterpret_cast<f32x4*>(out), n / 4);
    return viai_launch_status();
}

extern "C" int viai_outer_fwd(const float* x, const float* w, const float* b, float* y, long rows, int C, void* stream) {
    if (C % 4 != 0) return (int)hipErrorInvalidValue;
    VIAI_LAUNCH(outer_fwd_kernel, dim3(ew_blocks(rows * (C / 4))), dim3(256), 0, (hipStream_t)stream, x, w, b, y, rows, C);
    return viai_launch_status();
}

extern "C" int viai_outer_bwd_blocks(long rows) { long b = (rows + 1023) / 1024; if (b > 1024) b = 1024; if (b < 1) b = 1; return (int)b; }

extern "C" int viai_outer_bwd(const float* dy, const float* x, float* part, float* dw, float* db, long rows, int C, int accumulate, void* stream) {
    if (C % 4 != 0) return (int)hipErrorInvalidValue;
    int nb = viai_outer_bwd_blocks(rows);
    long rpb = (rows + nb - 1) / nb;
    VIAI_LAUNCH(outer_bwd_part_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, dy, x, part, rows, C, rpb);
    VIAI_LAUNCH(outer_bwd_final_kernel, dim3((C + 255) / 256), dim3(256), 0, (hipStream_t)stream, part, nb, C, dw, db, accumulate);
    return viai_launch_status();
}

extern "C" int viai_upsample_fwd(const float* x, const float* w, const float* bias, float* y, int B, int F, int T, int KH, int S, void* stream) {
    if (KH != 3 && KH != 1) return (int)hipErrorInvalidValue;
    long BF = (long)B * F;
    int blocks = ew_blocks(BF * T * S);
    if (KH == 3) VIAI_LAUNCH(upsample_fwd_kernel<3>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, w, bias, y, BF, F, T, S);
    else VIAI_LAUNCH(upsample_fwd_kernel<1>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, w, bias, y, BF, F, T, S);
    return viai_launch_status();
}

extern "C" int viai_upsample_bwd_blocks(void) { return 512; }

extern "C" int viai_upsample_bwd(const float* dy, const float* y, const float* x, const float* w, float* part, float* dx, float* dw, float* db,
                                 int B, int F, int T, int KH, int S, int accumulate, void* stream) {
    if ((KH != 3 && KH != 1) || S > 16) return (int)hipErrorInvalidValue;
    long BF = (long)B * F;
    hipStream_t st = (hipStream_t)stream;
    const int nb = 512;
    if (KH == 3) {
        if (dx) VIAI_LAUNCH(upsample_bwd_x_kernel<3>, dim3(ew_blocks(BF * T)), dim3(256), 0, st, dy, y, w, dx, BF, F, T, S);
        VIAI_LAUNCH(upsample_bwd_w_kernel<3>, dim3(nb), dim3(256), 0, st, dy, y, x, part, BF, F, T, S);
    } else {
        if (dx) VIAI_LAUNCH(upsample_bwd_x_kernel<1>, dim3(ew_blocks(BF * T)), dim3(256), 0, st, dy, y, w, dx, BF, F, T, S);
        VIAI_LAUNCH(upsample_bwd_w_kernel<1>, dim3(nb), dim3(256), 0, st, dy, y, x, part, BF, F, T, S);
    }
    VIAI_LAUNCH(upsample_bwd_final_kernel, dim3(1), dim3(64), 0, st, part, nb, KH, S, dw, db, accumulate);
    return viai_launch_status();
}

extern "C" int viai_mol_loss(const float* yhat, const float* y, const float* mask, float* loss_rows, float* wrow, float* loss,
                             float* dyhat, long rows, int pitch, int nr_mix, float num_classes, float log_scale_min, void* stream) {
    if (nr_mix != 10 || pitch < 30) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    // pass 1: per-row losses; masked mean + normalised row weights; pass 2 (if dyhat): gradients with those weights
    VIAI_LAUNCH(mol_loss_kernel<10>, dim3(ew_blocks(rows)), dim3(256), 0, st, yhat, y, (const float*)nullptr, loss_rows, (float*)nullptr, rows, pitch, num_classes, log_scale_min);
    VIAI_LAUNCH(masked_mean_kernel, dim3(1), dim3(256), 0, st, loss_rows, mask, rows, loss, wrow);
    if (dyhat) VIAI_LAUNCH(mol_loss_kernel<10>, dim3(ew_blocks(rows)), dim3(256), 0, st, yhat, y, wrow, loss_rows, dyhat, rows, pitch, num_classes, log_scale_min);
    return viai_launch_status();
}

template <int NV>
static void masked_ce_launch(const float* logits, const int* target, const float* mask, float* loss_rows, float* wrow, float* loss,
                             float* dlogits, long rows, int T, int K, int pitch, int shift, hipStream_t st) {
    const long nb = (rows + 3) / 4;
    const int blocks = (int)(nb > 16384 ? 16384 : (nb < 1 ? 1 : nb));
    float* meff = wrow + rows;
    // pass 1: per-row losses; masked mean + normalised row weights in a fixed order; pass 2 (if dlogits): gradients with those weights
    VIAI_LAUNCH(masked_ce_rows_kernel<NV>, dim3(blocks), dim3(256), 0, st, logits, target, mask, loss_rows, meff, rows, T, K, pitch, shift);
    VIAI_LAUNCH(masked_mean_kernel, dim3(1), dim3(256), 0, st, (const float*)loss_rows, (const float*)meff, rows, loss, wrow);
    if (dlogits) VIAI_LAUNCH(masked_ce_grad_kernel<NV>, dim3(blocks), dim3(256), 0, st, logits, target, (const float*)wrow, dlogits, rows, T, K, pitch, shift);
}

extern "C" int viai_masked_ce_loss(const float* logits, const int* target, const float* mask, float* loss_rows, float* wrow, float* loss,
                                   float* dlogits, int B, int T, int K, int pitch, int shift, void* stream) {
    if (B < 1 || T < 1 || K < 4 || K % 4 != 0 || pitch < K || pitch % 4 != 0 || K > 256 * CE_MAXV || shift < 0 || shift >= T)
        return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    const long rows = (long)B * T;
    switch ((K + 255) / 256) {
        case 1: masked_ce_launch<1>(logits, target, mask, loss_rows, wrow, loss, dlogits, rows, T, K, pitch, shift, st); break;
        case 2: masked_ce_launch<2>(logits, target, mask, loss_rows, wrow, loss, dlogits, rows, T, K, pitch, shift, st); break;
        case 3: masked_ce_launch<3>(logits, target, mask, loss_rows, wrow, loss, dlogits, rows, T, K, pitch, shift, st); break;
        default: masked_ce_launch<4>(logits, target, mask, loss_rows, wrow, loss, dlogits, rows, T, K, pitch, shift, st); break;
    }
    return viai_launch_status();
}

extern "C" int viai_class_embed_fwd(const int* classes, const float* w, const float* b, float* wt, float* h, long rows, int K, int C, void* stream) {
    if (rows < 1 || K < 1 || C < 4 || C % 4 != 0) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    VIAI_LAUNCH(transpose_kernel, dim3((K + 31) / 32, (C + 31) / 32), dim3(256), 0, st, w, wt, C, K);
    VIAI_LAUNCH(class_embed_fwd_kernel, dim3(ew_blocks(rows * (C / 4))), dim3(256), 0, st, classes, reinterpret_cast<const f32x4*>(wt),
                reinterpret_cast<const f32x4*>(b), reinterpret_cast<f32x4*>(h), rows, K, C / 4);
    return viai_launch_status();
}

// row segments of the weight gradient: 2048 rows each (one chunk), at most 64 of them
extern "C" int viai_class_embed_bwd_segments(long rows) {
    long s = (rows + CEB_CHUNK - 1) / CEB_CHUNK;
    if (s > 64) s = 64;
    if (s < 1) s = 1;
    return (int)s;
}

extern "C" int viai_class_embed_bwd(const float* dh, const int* classes, float* part, float* dw, float* db, long rows, int K, int C, void* stream) {
    if (rows < 1 || K < 1 || K > 65535 || C < 4 || C % 4 != 0 || C > 1024) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    const int S = viai_class_embed_bwd_segments(rows);
    long seg = (rows + S - 1) / S;
    seg = (seg + CEB_CHUNK - 1) / CEB_CHUNK * CEB_CHUNK;               // whole chunks, so a chunk never straddles two segments
    VIAI_LAUNCH(class_embed_bwd_part_kernel, dim3(K, S), dim3(256), 0, st, dh, classes, part, rows, seg, K, C);
    VIAI_LAUNCH(class_embed_final_kernel, dim3((C + 31) / 32, (K + 31) / 32), dim3(256), 0, st, (const float*)part, dw, S, K, C);
    VIAI_LAUNCH(class_embed_bias_kernel, dim3(C), dim3(256), 0, st, (const float*)dw, db, K);
    return viai_launch_status();
}

extern "C" int viai_mulaw_quantize(const float* x, int* classes, long n, int mu, void* stream) {
    if (n < 1 || mu < 1) return (int)hipErrorInvalidValue;
    VIAI_LAUNCH(mulaw_quantize_kernel, dim3(ew_blocks(n)), dim3(256), 0, (hipStream_t)stream, x, classes, n, (float)mu);
    return viai_launch_status();
}

extern "C" int viai_scale_by_scalar(float* d, const float* gscale, long n, void* stream) {
    VIAI_LAUNCH(scale_rows_kernel, dim3(ew_blocks(n)), dim3(256), 0, (hipStream_t)stream, d, gscale, n);
    return viai_launch_status();
}

extern "C" int viai_mol_sample(const float* yhat, const float* u1, const float* u2, float* out, long rows, int pitch, int nr_mix,
                               float log_scale_min, void* stream) {
    if (nr_mix != 10) return (int)hipErrorInvalidValue;
    VIAI_LAUNCH(mol_sample_kernel<10>, dim3(ew_blocks(rows)), dim3(256), 0, (hipStream_t)stream, yhat, u1, u2, out, rows, pitch, log_scale_min);
    return viai_launch_status();
}

// =====================================================================================================
// Incremental synthesis (wavenet.py:237-364, conv.py:17-46).  One time step = first conv + per layer two
// GEMV-batch kernels (gate, then out/skip) + head (two 1x1 layers + MoL sample).  The time index lives in
// DEVICE memory (`step`), ring-buffer slots are derived from it inside the kernels, so every launch has static
// arguments and one step can be captured once into a hipGraph and replayed T times.
// Linearised weights: Wlin[g][j*C + ci] = w[g][ci][j] (conv.py:53-57), taps j = 0..2 read x[t-(2-j)*d].
namespace {

constexpr int WN_MAXB = 8;

// A stream's arithmetic must not depend on how many streams travel with it: the kernels below are templates over the stream count NB, and with
// floating-point contraction left to the compiler each instantiation fused another subset of the products into its sums (it packs the streams
// pairwise: wn_out_kernel<1> had no fused multiply-add, <2> had), so stream b of a 4-stream run differed in the last bits from the 1-stream run
// on the same inputs.  WN_STRICT_FP, first statement of every NB-templated kernel, switches contraction off there: every product and sum is
// rounded on its own, in source order, whatever NB is.
#define WN_STRICT_FP _Pragma("clang fp contract(off)")

// Is the input of time step t of stream b given (teacher-forced)?  Without a mask: the common prefix t < n_test (wavenet.py:322-323).  With a
// mask `forced` (B, T) uint8 (viai_wavenet_synth_run_forced; the test inputs then cover all T steps, n_test == T): the mask's entry.
__device__ __forceinline__ bool wn_forced(const unsigned char* __restrict__ forced, int n_test, int T, int t, int b) {
    return forced != nullptr ? forced[(size_t)b * T + t] != 0 : t < n_test;
}

// x0[b][:] = cur[b] * w_first + b_first -> ring0[slot(t)];  cur = test_inputs[t] | out[t-1] | 0
// ONE block.  The time index comes either by value (t_arg >= 0: viai_wavenet_synth_run, the host loop knows it) or from device memory
// (t_arg < 0: viai_wavenet_synth_step, replayable from a hipGraph): there this kernel also advances it once all of its threads have
// read it -- `*step` counts the first-conv launches, the other kernels of the time step read t = *step - 1 (a separate one-thread
// tick launch cost 4.3 us per time step).  A load of the index is a full memory round trip (~1.5 us at these tiny grids) in FRONT of
// every address computation of every kernel, which is why the by-value path exists.
__global__ __launch_bounds__(256) void wn_first_kernel(const float* __restrict__ w, const float* __restrict__ bias, const float* __restrict__ test_inputs,
                                                       int n_test, const float* __restrict__ out, float* __restrict__ ring, int ring_len,
                                                       int* __restrict__ step, int t_arg, int B, int C, int T,
                                                       const unsigned char* __restrict__ forced) {
    const int t = t_arg >= 0 ? t_arg : *step;
    const int slot = t % ring_len;
    for (int i = threadIdx.x; i < B * C; i += 256) {
        int b = i / C, c = i % C;
        float cur = wn_forced(forced, n_test, T, t, b) ? test_inputs[(size_t)b * n_test + t] : (t > 0 ? out[(size_t)b * T + t - 1] : 0.f);
        ring[((size_t)b * ring_len + slot) * C + c] = cur * w[c] + bias[c];
    }
    if (t_arg < 0) {
        __syncthreads();
        if (threadIdx.x == 0) *step = t + 1;
    }
}

// gate: z[b][h] = tanh(A) * sigmoid(Bv),  A/Bv = rows h / h+H of (Wlin . [x(t-2d); x(t-d); x(t)] + b + Wc . c_t + bc)
// One BLOCK per output pair (h, h+H): the 3C + cin reduction is cut into 16-byte chunks over the 256 threads (reference size:
// 384 + 20 chunks, at most two per thread, all loads of a thread in flight at once), the 2 x NB partial sums meet in LDS.
// (The first version gave a WAVE the whole row: six dependent trips of 10 loads per lane on 64 blocks, 10.8 us per launch.)
template <int NB>
__global__ __launch_bounds__(256) void wn_gate_kernel(const float* __restrict__ ring, int ring_len, int dil, const float* __restrict__ wlin,
                                                      const float* __restrict__ bconv, const float* __restrict__ wc, const float* __restrict__ bc,
                                                      const float* __restrict__ cond, const float* __restrict__ gadd, float* __restrict__ z,
                                                      const int* __restrict__ step, int t_arg, int C, int H, int cin, int T) {
    WN_STRICT_FP
    __shared__ float red[2 * NB][260];
    const int t = t_arg >= 0 ? t_arg : *step - 1;
    const int h = blockIdx.x, tid = threadIdx.x;
    // the epilogue's biases are fetched now, not after the reduction (one memory round trip less on the critical path)
    float ba = 0.f, bg = 0.f;
    if ((tid & 31) == 0 && tid < 32 * NB) {
        ba = bconv[h] + (bc ? bc[h] : 0.f); bg = bconv[h + H] + (bc ? bc[h + H] : 0.f);
        if (gadd != nullptr) { ba += gadd[(size_t)(tid >> 5) * 2 * H + h]; bg += gadd[(size_t)(tid >> 5) * 2 * H + h + H]; }
    }
    const int K = 3 * C;
    const int nq = K / 4, nqc = wc != nullptr ? cin / 4 : 0;
    float a[NB], g[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) { a[b] = 0.f; g[b] = 0.f; }
    const float* wa = wlin + (size_t)h * K;
    const float* wg = wlin + (size_t)(h + H) * K;
    for (int q = tid; q < nq + nqc; q += 256) {
        f32x4 va, vg;
        const float* xb;
        size_t xstride;
        bool live = true;
        if (q < nq) {
            const int k = q * 4;
            const int j = k / C, ci = k - j * C;
            const int tt = t - (2 - j) * dil;
            live = tt >= 0;
            va = *reinterpret_cast<const f32x4*>(wa + k); vg = *reinterpret_cast<const f32x4*>(wg + k);
            xb = ring + (size_t)(live ? tt % ring_len : 0) * C + ci;
            xstride = (size_t)ring_len * C;
        } else {
            const int k = (q - nq) * 4;
            va = *reinterpret_cast<const f32x4*>(wc + (size_t)h * cin + k); vg = *reinterpret_cast<const f32x4*>(wc + (size_t)(h + H) * cin + k);
            xb = cond + (size_t)t * cin + k;
            xstride = (size_t)T * cin;
        }
        if (live) {
            f32x4 x[NB];
#pragma unroll
            for (int b = 0; b < NB; ++b) x[b] = *reinterpret_cast<const f32x4*>(xb + b * xstride);
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                a[b] += x[b][0] * va[0] + x[b][1] * va[1] + x[b][2] * va[2] + x[b][3] * va[3];
                g[b] += x[b][0] * vg[0] + x[b][1] * vg[1] + x[b][2] * vg[2] + x[b][3] * vg[3];
            }
        }
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) { red[2 * b][tid] = a[b]; red[2 * b + 1][tid] = g[b]; }
    __syncthreads();
    // 16 lanes per value: lane `part` adds 16 of the 256 partials, four butterfly steps finish the sum (fixed order)
    if (tid < 32 * NB) {
        const int v = tid >> 4, part = tid & 15;
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < 16; ++j) sum += red[v][part * 16 + ((j + part) & 15)];
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
        const float other = __shfl_down(sum, 16, 64);          // the gate half (value 2b + 1) sits 16 lanes up
        if ((tid & 31) == 0) {
            const int b = tid >> 5;
            const float sa = sum + ba, sg = other + bg;
            z[(size_t)b * H + h] = tanhf(sa) * (1.f / (1.f + expf(-sg)));
        }
    }
}

// out/skip: o < C: x_next[b][o] = (Wout[o].z + bout[o] + x_t[b][o]) * sqrt(.5) -> next ring;  o >= C: skip accumulate
template <int NB>
__global__ __launch_bounds__(256) void wn_out_kernel(const float* __restrict__ z, const float* __restrict__ wout, const float* __restrict__ bout,
                                                     const float* __restrict__ wskip, const float* __restrict__ bskip,
                                                     const float* __restrict__ ring, int ring_len, float* __restrict__ next_ring, int next_len,
                                                     float* __restrict__ skips, int first, const int* __restrict__ step, int t_arg, int C, int H, int S) {
    WN_STRICT_FP
    const int t = t_arg >= 0 ? t_arg : *step - 1;
    const int o = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (o >= C + S) return;
    const float* w = o < C ? wout + (size_t)o * H : wskip + (size_t)(o - C) * H;
    // what the epilogue adds (residual x_t / running skip sum, bias) is fetched NOW by lane b for stream b, beside the dot
    // products, instead of after the reduction
    float pre = 0.f;
    if (lane < NB) pre = o < C ? ring[((size_t)lane * ring_len + (t % ring_len)) * C + o] : (first ? 0.f : skips[(size_t)lane * S + (o - C)]);
    const float bias = o < C ? bout[o] : bskip[o - C];
    float acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[b] = 0.f;
    for (int k = lane * 4; k < H; k += 256) {
        const f32x4 wv = *reinterpret_cast<const f32x4*>(w + k);
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(z + (size_t)b * H + k);
            acc[b] += x[0] * wv[0] + x[1] * wv[1] + x[2] * wv[2] + x[3] * wv[3];
        }
    }
    const float r5 = 0.70710678118654752f;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const float v = wave_sum_dpp(acc[b]);
        const float p = __shfl(pre, b, 64);
        if (lane == 0) {
            if (o < C) {
                if (next_ring) next_ring[((size_t)b * next_len + (t % next_len)) * C + o] = (v + bias + p) * r5;
            } else {
                const float sv = v + bias;
                skips[(size_t)b * S + (o - C)] = first ? sv : (p + sv) * r5;
            }
        }
    }
}

// head: relu -> W1 -> relu -> W2 -> MoL sample with injected uniforms -> out[b][t]; one block of 16 waves per stream.
// At one block per stream the kernel is a chain of load latencies, so everything that does not depend on the previous stage is
// fetched up front (uniforms, biases) and every stage has all of its rows in flight at once: a wave takes 16 rows, each read
// coalesced (16 bytes per lane).  (A row per THREAD, 256 strided loads in sequence: 17.7 us; four rows per trip: 49 us.)
__global__ __launch_bounds__(1024) void wn_head_kernel(const float* __restrict__ skips, const float* __restrict__ w1, const float* __restrict__ b1,
                                                       const float* __restrict__ w2, const float* __restrict__ b2, const float* __restrict__ u1,
                                                       const float* __restrict__ u2, float* __restrict__ out, float* __restrict__ yhat_dbg,
                                                       const int* __restrict__ step, int t_arg, int S, int OC, int T, float log_scale_min) {
    extern __shared__ __attribute__((aligned(16))) float sm[];          // [S] relu(skips), [S] hidden, [OC] logits, [OC/3 + 1] uniforms
    float* xin = sm; float* hid = sm + S; float* yo = sm + 2 * S; float* us = yo + ((OC + 3) & ~3);
    const int b = blockIdx.x, tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    constexpr int RB = 16;
    const int K = OC / 3;
    // Stage order = what can be in flight together: W1's rows depend on nothing, so they (and the biases) are requested before the
    // time index or the skip sums arrive; W2's rows are requested as soon as W1's registers are free, i.e. before W1's reductions
    // and the barrier.  A wave holds ONE 16-row batch at a time (16 waves at 128 registers each: holding both layers spilt to scratch,
    // 38 us per launch).  Needs S <= 256 and out_ch <= 256 (the reference: 256 / 30); wn_head_generic_kernel takes anything else.
    const int k0 = lane * 4;
    const int r1 = wave * RB, r2 = wave * RB;
    const float bv1 = b1[min(r1 + (lane & (RB - 1)), S - 1)], bv2 = b2[min(r2 + (lane & (RB - 1)), OC - 1)];
    f32x4 p[RB];
    if (r1 < S && k0 < S) {
#pragma unroll
        for (int r = 0; r < RB; ++r) p[r] = *reinterpret_cast<const f32x4*>(w1 + (size_t)min(r1 + r, S - 1) * S + k0);
    }
    const int t = t_arg >= 0 ? t_arg : *step - 1;
    for (int k = tid; k < S; k += 1024) { float v = skips[(size_t)b * S + k]; xin[k] = v > 0.f ? v : 0.f; }
    if (tid < K) us[tid] = u1[((size_t)b * T + t) * K + tid];
    if (tid == K) us[K] = u2[(size_t)b * T + t];
    __syncthreads();
    // one 16-row batch: acc[r] = row (r0 + r) . x with the row slices already in registers (S <= 256: one 16-byte slice per lane)
    auto batch = [&](const float* __restrict__, const f32x4 (&pre)[RB], const float* x, int, float (&acc)[RB]) {
        const f32x4 xv = k0 < S ? *reinterpret_cast<const f32x4*>(x + k0) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < RB; ++r) acc[r] = k0 < S ? pre[r][0] * xv[0] + pre[r][1] * xv[1] + pre[r][2] * xv[2] + pre[r][3] * xv[3] : 0.f;
    };
    auto finish = [&](const float (&acc)[RB], float bv, int h0, int n_out, auto&& emit) {
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            const float v = wave_sum_dpp(acc[r]) + __shfl(bv, r, 64);
            if (lane == 0 && h0 + r < n_out) emit(h0 + r, v);
        }
    };
    auto hid_out = [&](int h, float v) { hid[h] = v > 0.f ? v : 0.f; };
    auto logit_out = [&](int o, float v) { yo[o] = v; if (yhat_dbg) yhat_dbg[((size_t)b * T + t) * OC + o] = v; };
    float acc[RB];
    if (r1 < S) batch(w1, p, xin, S, acc);
    if (r2 < OC && k0 < S) {                                   // W2's first batch: in flight across W1's reductions and the barrier
#pragma unroll
        for (int r = 0; r < RB; ++r) p[r] = *reinterpret_cast<const f32x4*>(w2 + (size_t)min(r2 + r, OC - 1) * S + k0);
    }
    if (r1 < S) finish(acc, bv1, r1, S, hid_out);
    __syncthreads();
    if (r2 < OC) { batch(w2, p, hid, OC, acc); finish(acc, bv2, r2, OC, logit_out); }
    __syncthreads();
    if (tid == 0) {
        float best = -INFINITY; int arg = 0;
        for (int k = 0; k < K; ++k) {
            float v = yo[k] - logf(-logf(us[k]));
            if (v > best) { best = v; arg = k; }
        }
        const float m = yo[K + arg], ls = fmaxf(yo[2 * K + arg], log_scale_min), u = us[K];
        float x = m + expf(ls) * (logf(u) - logf(1.f - u));
        out[(size_t)b * T + t] = fminf(fmaxf(x, -1.f), 1.f);
    }
}

// any S / out_ch: a row per thread (the first version of the head)
__global__ __launch_bounds__(256) void wn_head_generic_kernel(const float* __restrict__ skips, const float* __restrict__ w1, const float* __restrict__ b1,
                                                              const float* __restrict__ w2, const float* __restrict__ b2, const float* __restrict__ u1,
                                                              const float* __restrict__ u2, float* __restrict__ out, float* __restrict__ yhat_dbg,
                                                              const int* __restrict__ step, int t_arg, int S, int OC, int T, float log_scale_min) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* xin = sm; float* hid = sm + S; float* yo = sm + 2 * S;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int t = t_arg >= 0 ? t_arg : *step - 1;
    for (int k = tid; k < S; k += 256) { float v = skips[(size_t)b * S + k]; xin[k] = v > 0.f ? v : 0.f; }
    __syncthreads();
    for (int h = tid; h < S; h += 256) {
        float acc = b1[h];
        for (int k = 0; k < S; ++k) acc += w1[(size_t)h * S + k] * xin[k];
        hid[h] = acc > 0.f ? acc : 0.f;
    }
    __syncthreads();
    for (int o = tid; o < OC; o += 256) {
        float acc = b2[o];
        for (int k = 0; k < S; ++k) acc += w2[(size_t)o * S + k] * hid[k];
        yo[o] = acc;
        if (yhat_dbg) yhat_dbg[((size_t)b * T + t) * OC + o] = acc;
    }
    __syncthreads();
    if (tid == 0) {
        const int K = OC / 3;
        float best = -INFINITY; int arg = 0;
        for (int k = 0; k < K; ++k) {
            float v = yo[k] - logf(-logf(u1[((size_t)b * T + t) * K + k]));
            if (v > best) { best = v; arg = k; }
        }
        const float m = yo[K + arg], ls = fmaxf(yo[2 * K + arg], log_scale_min), u = u2[(size_t)b * T + t];
        float x = m + expf(ls) * (logf(u) - logf(1.f - u));
        out[(size_t)b * T + t] = fminf(fmaxf(x, -1.f), 1.f);
    }
}

// ---- fused stages (ABI 7): ONE dependent launch per layer instead of two -----------------------------------------------------------
// A time step of the plain form is a chain of 2 L + 2 dependent launches: gate_l needs all of x_l(t), which out_{l-1} produces from all
// of z_{l-1}.  But x_l(t) = (Wo_{l-1} z_{l-1} + bo_{l-1} + x_{l-1}(t)) sqrt(.5) is LINEAR in z_{l-1}, and gate_l uses it only through
// the current tap Wc_l^2 x_l(t), so
//     Wc_l^2 x_l(t) = [sqrt(.5) Wc_l^2 Wo_{l-1}] z_{l-1} + [sqrt(.5) Wc_l^2] x_{l-1}(t) + sqrt(.5) Wc_l^2 bo_{l-1}
// and gate_l can start from what stage l - 1 left behind: z_{l-1} and x_{l-1}(t).  The host builds the extended rows
// [Wc^0 | Wc^1 | sqrt(.5) Wc^2 | sqrt(.5) Wc^2 Wo_{l-1}] (K = 3 C + H) and the folded bias once; stage l then runs, side by side in
// one launch, (A) gate_l -> z_l from the two past taps (ring_l), x_{l-1}(t) (ring_{l-1}) and z_{l-1}, and (B) the out / skip rows of
// layer l - 1 (x_l(t) -> ring_l for the FUTURE time steps' past taps, the running skip sum).  Stage 0 forms x_0(t) = first conv inline.
// The last layer's skip row product moves into the head.  L + 1 dependent launches per time step; z is double-buffered (stage l
// writes z_l while its B blocks still read z_{l-1}).  Reassociation only: sums agree with the plain form to fp32 rounding.
// ---- categorical network (ABI 19): where the input of a time step comes from (wavenet.py:322-327), shared by both chain forms --------------
// Two forms of the first conv (wavenet.py:116-119, Conv1d1x1(K, C)): the input of stream b is a CLASS k -> x0 = w_t[k] + bias, one contiguous
// row of the transposed weight; or a DENSE row of K floats -> x0[c] = w[c] . row + bias[c].  The form of a STEP depends on t, the descriptor
// and (where there is one) the mask of forced steps, never on the block, so every branch on it is uniform over the grid.
struct WnCatIn {
    const float* w_t; const float* w;              // [K][C] / [C][K]
    const int* test_classes; const float* test_rows; const float* init_rows;
    const int* classes; const float* rows;         // what the previous time steps put out: (B, T) / (B, T, K)
    int n_test, init_class, quantize, K, T;
    const unsigned char* forced;                   // optional (B, T) mask of the teacher-forced steps (wn_forced)
};

// the form of stream b's input at step t; without a mask it is the same for every stream
__device__ __forceinline__ bool wn_cat_class_form_of(const WnCatIn& in, int t, int b) {
    if (wn_forced(in.forced, in.n_test, in.T, t, b)) return in.test_classes != nullptr;
    if (t > 0) return in.quantize != 0;
    return in.init_rows == nullptr;
}
// the form of the STEP: class form only if every stream's input is a class.  With a mask the streams may differ (one forced from dense rows,
// one fed back as a class): such a step takes the dense path, where a class stream still gathers its row (wn_cat_first_kernel).  The answer
// depends on t, the descriptor and the mask only, so every branch on it is uniform over the grid.
template <int NB>
__device__ __forceinline__ bool wn_cat_class_form(const WnCatIn& in, int t) {
    if (in.forced == nullptr) return wn_cat_class_form_of(in, t, 0);
    bool all = true;
#pragma unroll
    for (int b = 0; b < NB; ++b) all = all && wn_cat_class_form_of(in, t, b);
    return all;
}
__device__ __forceinline__ int wn_cat_class(const WnCatIn& in, int t, int b) {
    const int k = wn_forced(in.forced, in.n_test, in.T, t, b) ? in.test_classes[(size_t)b * in.n_test + t]
                                                              : (t > 0 ? in.classes[(size_t)b * in.T + t - 1] : in.init_class);
    return min(max(k, 0), in.K - 1);               // a class from outside (test_classes) never indexes past the weight
}
__device__ __forceinline__ const float* wn_cat_row(const WnCatIn& in, int t, int b) {
    return wn_forced(in.forced, in.n_test, in.T, t, b) ? in.test_rows + ((size_t)b * in.n_test + t) * in.K
                                                       : (t > 0 ? in.rows + ((size_t)b * in.T + t - 1) * in.K : in.init_rows + (size_t)b * in.K);
}

struct WnStage {
    WnCatIn cat;                                   // categorical network, stage 0 (wn_stage_kernel<NB, true>)
    const float* ring; int ring_len, dil;          // x_l at the past time steps
    const float* ring_prev; int prev_len;          // x_{l-1}, current slot written by stage l - 1 (l > 0)
    const float* w; const float* bias;             // [G][K] extended rows, [G] folded bias
    const float* wc; const float* cond; const float* gadd;
    const float* z_in; float* z_out;
    const float* w_first; const float* b_first; const float* test_inputs; int n_test; const float* out;   // stage 0
    const float* w_out; const float* b_out; const float* w_skip; const float* b_skip;                      // layer l - 1 (B blocks)
    float* ring_w; float* skips; int first_skip;
    const int* step; int t_arg, l, C, H, S, cin, T, B;
    const unsigned char* forced;                   // stage 0 of the scalar-input network: wn_forced
};

__global__ void wn_tick_kernel(int* step) { *step += 1; }

// CAT: the categorical network.  Stage 0 forms x_0(t) from a class by the gather above; a dense input row is a K-long product per channel, which
// wn_cat_first_kernel does in a launch of its own in front of this stage (ring slot t), and stage 0 reads its current tap from there.
template <int NB, bool CAT = false>
__global__ __launch_bounds__(256) void wn_stage_kernel(const WnStage a) {
    WN_STRICT_FP
    __shared__ float red[2 * NB][260];
    const int t = a.t_arg >= 0 ? a.t_arg : *a.step - 1;
    const int tid = threadIdx.x, C = a.C, H = a.H;
    if ((int)blockIdx.x >= H) {
        // ---------------------------------------------------------------- B: what layer l - 1 still owes (or the first conv)
        const int bid = blockIdx.x - H;
        if (CAT && a.l == 0) {
            if (wn_cat_class_form<NB>(a.cat, t))
                for (int i = tid; i < NB * C; i += 256) {
                    const int b = i / C, c = i - b * C;
                    a.ring_w[((size_t)b * a.ring_len + (t % a.ring_len)) * C + c] = a.cat.w_t[(size_t)wn_cat_class(a.cat, t, b) * C + c] + a.b_first[c];
                }
            return;
        }
        if (a.l == 0) {
            for (int i = tid; i < NB * C; i += 256) {
                const int b = i / C, c = i - b * C;
                const float cur = wn_forced(a.forced, a.n_test, a.T, t, b) ? a.test_inputs[(size_t)b * a.n_test + t] : (t > 0 ? a.out[(size_t)b * a.T + t - 1] : 0.f);
                a.ring_w[((size_t)b * a.ring_len + (t % a.ring_len)) * C + c] = cur * a.w_first[c] + a.b_first[c];
            }
            return;
        }
        const int o = bid * 4 + (tid >> 6), lane = tid & 63, S = a.S;
        if (o >= C + S) return;
        const float* w = o < C ? a.w_out + (size_t)o * H : a.w_skip + (size_t)(o - C) * H;
        float pre = 0.f;
        if (lane < NB) pre = o < C ? a.ring_prev[((size_t)lane * a.prev_len + (t % a.prev_len)) * C + o] : (a.first_skip ? 0.f : a.skips[(size_t)lane * S + (o - C)]);
        const float bias = o < C ? a.b_out[o] : a.b_skip[o - C];
        float acc[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[b] = 0.f;
        for (int k = lane * 4; k < H; k += 256) {
            const f32x4 wv = *reinterpret_cast<const f32x4*>(w + k);
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                const f32x4 x = *reinterpret_cast<const f32x4*>(a.z_in + (size_t)b * H + k);
                acc[b] += x[0] * wv[0] + x[1] * wv[1] + x[2] * wv[2] + x[3] * wv[3];
            }
        }
        const float r5 = 0.70710678118654752f;
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const float v = wave_sum_dpp(acc[b]);
            const float p = __shfl(pre, b, 64);
            if (lane == 0) {
                if (o < C) a.ring_w[((size_t)b * a.ring_len + (t % a.ring_len)) * C + o] = (v + bias + p) * r5;
                else { const float sv = v + bias; a.skips[(size_t)b * S + (o - C)] = a.first_skip ? sv : (p + sv) * r5; }
            }
        }
        return;
    }
    // -------------------------------------------------------------------- A: gate pair (h, h + H) of layer l
    const int h = blockIdx.x;
    float ba = 0.f, bg = 0.f;
    if ((tid & 31) == 0 && tid < 32 * NB) {
        ba = a.bias[h]; bg = a.bias[h + H];
        if (a.gadd != nullptr) { ba += a.gadd[(size_t)(tid >> 5) * 2 * H + h]; bg += a.gadd[(size_t)(tid >> 5) * 2 * H + h + H]; }
    }
    const int K = 3 * C + (a.l > 0 ? H : 0);
    const int nq = K / 4, nqc = a.wc != nullptr ? a.cin / 4 : 0;
    float sa[NB], sg[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) { sa[b] = 0.f; sg[b] = 0.f; }
    const float* wa = a.w + (size_t)h * K;
    const float* wg = a.w + (size_t)(h + H) * K;
    for (int q = tid; q < nq + nqc; q += 256) {
        f32x4 va, vg, x[NB];
        bool live = true;
        if (q < nq) {
            const int k = q * 4;
            va = *reinterpret_cast<const f32x4*>(wa + k); vg = *reinterpret_cast<const f32x4*>(wg + k);
            if (k < 2 * C) {                                        // past taps: x_l(t - 2 d), x_l(t - d)
                const int j = k / C, ci = k - j * C;
                const int tt = t - (2 - j) * a.dil;
                live = tt >= 0;
                if (live) {
                    const float* xb = a.ring + (size_t)(tt % a.ring_len) * C + ci;
#pragma unroll
                    for (int b = 0; b < NB; ++b) x[b] = *reinterpret_cast<const f32x4*>(xb + (size_t)b * a.ring_len * C);
                }
            } else if (k < 3 * C) {                                 // current tap
                const int ci = k - 2 * C;
                if (CAT && a.l == 0) {                              // x_0(t) of the categorical network
                    if (wn_cat_class_form<NB>(a.cat, t)) {
                        const f32x4 bf = *reinterpret_cast<const f32x4*>(a.b_first + ci);
#pragma unroll
                        for (int b = 0; b < NB; ++b) x[b] = *reinterpret_cast<const f32x4*>(a.cat.w_t + (size_t)wn_cat_class(a.cat, t, b) * C + ci) + bf;
                    } else {
                        const float* xb = a.ring + (size_t)(t % a.ring_len) * C + ci;
#pragma unroll
                        for (int b = 0; b < NB; ++b) x[b] = *reinterpret_cast<const f32x4*>(xb + (size_t)b * a.ring_len * C);
                    }
                } else if (a.l == 0) {                              // x_0(t): the first conv, formed here
                    const f32x4 wf = *reinterpret_cast<const f32x4*>(a.w_first + ci), bf = *reinterpret_cast<const f32x4*>(a.b_first + ci);
#pragma unroll
                    for (int b = 0; b < NB; ++b) {
                        const float cur = wn_forced(a.forced, a.n_test, a.T, t, b) ? a.test_inputs[(size_t)b * a.n_test + t] : (t > 0 ? a.out[(size_t)b * a.T + t - 1] : 0.f);
                        x[b] = cur * wf + bf;
                    }
                } else {                                            // x_{l-1}(t), against sqrt(.5) Wc^2
                    const float* xb = a.ring_prev + (size_t)(t % a.prev_len) * C + ci;
#pragma unroll
                    for (int b = 0; b < NB; ++b) x[b] = *reinterpret_cast<const f32x4*>(xb + (size_t)b * a.prev_len * C);
                }
            } else {                                                // z_{l-1}, against sqrt(.5) Wc^2 Wo_{l-1}
                const int kz = k - 3 * C;
#pragma unroll
                for (int b = 0; b < NB; ++b) x[b] = *reinterpret_cast<const f32x4*>(a.z_in + (size_t)b * H + kz);
            }
        } else {
            const int k = (q - nq) * 4;
            va = *reinterpret_cast<const f32x4*>(a.wc + (size_t)h * a.cin + k); vg = *reinterpret_cast<const f32x4*>(a.wc + (size_t)(h + H) * a.cin + k);
            const float* xb = a.cond + (size_t)t * a.cin + k;
#pragma unroll
            for (int b = 0; b < NB; ++b) x[b] = *reinterpret_cast<const f32x4*>(xb + (size_t)b * a.T * a.cin);
        }
        if (live) {
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                sa[b] += x[b][0] * va[0] + x[b][1] * va[1] + x[b][2] * va[2] + x[b][3] * va[3];
                sg[b] += x[b][0] * vg[0] + x[b][1] * vg[1] + x[b][2] * vg[2] + x[b][3] * vg[3];
            }
        }
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) { red[2 * b][tid] = sa[b]; red[2 * b + 1][tid] = sg[b]; }
    __syncthreads();
    if (tid < 32 * NB) {
        const int v = tid >> 4, part = tid & 15;
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < 16; ++j) sum += red[v][part * 16 + ((j + part) & 15)];
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
        const float other = __shfl_down(sum, 16, 64);
        if ((tid & 31) == 0) {
            const int b = tid >> 5;
            const float va_ = sum + ba, vg_ = other + bg;
            a.z_out[(size_t)b * H + h] = tanhf(va_) * (1.f / (1.f + expf(-vg_)));
        }
    }
}

// head of the fused form: first the LAST layer's skip rows (skips <- (skips + Ws z + bs) sqrt(.5), relu'd into LDS), then wn_head_kernel's
// two layers and the sampler.  16 waves x 16 rows, S <= 256, H <= 256, out_ch <= 256.
__global__ __launch_bounds__(1024) void wn_head_fused_kernel(const float* __restrict__ skips, const float* __restrict__ z, const float* __restrict__ wsk,
                                                             const float* __restrict__ bsk, int first_skip, int H,
                                                             const float* __restrict__ w1, const float* __restrict__ b1,
                                                             const float* __restrict__ w2, const float* __restrict__ b2, const float* __restrict__ u1,
                                                             const float* __restrict__ u2, float* __restrict__ out, float* __restrict__ yhat_dbg,
                                                             const int* __restrict__ step, int t_arg, int S, int OC, int T, float log_scale_min) {
    extern __shared__ __attribute__((aligned(16))) float sm[];          // [S] relu(skips), [S] hidden, [OC] logits, [OC/3 + 1] uniforms
    float* xin = sm; float* hid = sm + S; float* yo = sm + 2 * S; float* us = yo + ((OC + 3) & ~3);
    const int b = blockIdx.x, tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    constexpr int RB = 16;
    const int K = OC / 3;
    const int k0 = lane * 4;
    const int r0 = wave * RB;
    f32x4 p[RB];
    if (r0 < S && k0 < H) {
#pragma unroll
        for (int r = 0; r < RB; ++r) p[r] = *reinterpret_cast<const f32x4*>(wsk + (size_t)min(r0 + r, S - 1) * H + k0);
    }
    const float bvs = bsk[min(r0 + (lane & (RB - 1)), S - 1)];
    const float bv1 = b1[min(r0 + (lane & (RB - 1)), S - 1)], bv2 = b2[min(r0 + (lane & (RB - 1)), OC - 1)];
    const float prev = (!first_skip && r0 < S) ? skips[(size_t)b * S + min(r0 + (lane & (RB - 1)), S - 1)] : 0.f;
    const int t = t_arg >= 0 ? t_arg : *step - 1;
    if (tid < K) us[tid] = u1[((size_t)b * T + t) * K + tid];
    if (tid == K) us[K] = u2[(size_t)b * T + t];
    float acc[RB];
    const float r5 = 0.70710678118654752f;
    if (r0 < S) {
        const f32x4 zv = k0 < H ? *reinterpret_cast<const f32x4*>(z + (size_t)b * H + k0) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < RB; ++r) acc[r] = k0 < H ? p[r][0] * zv[0] + p[r][1] * zv[1] + p[r][2] * zv[2] + p[r][3] * zv[3] : 0.f;
    }
    if (r0 < S && k0 < S) {                                    // W1's rows: in flight across the skip reductions
#pragma unroll
        for (int r = 0; r < RB; ++r) p[r] = *reinterpret_cast<const f32x4*>(w1 + (size_t)min(r0 + r, S - 1) * S + k0);
    }
    if (r0 < S) {
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            const float sv = wave_sum_dpp(acc[r]) + __shfl(bvs, r, 64);
            const float pv = __shfl(prev, r, 64);
            if (lane == 0 && r0 + r < S) { const float v = first_skip ? sv : (pv + sv) * r5; xin[r0 + r] = v > 0.f ? v : 0.f; }
        }
    }
    __syncthreads();
    if (r0 < S) {
        const f32x4 xv = k0 < S ? *reinterpret_cast<const f32x4*>(xin + k0) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < RB; ++r) acc[r] = k0 < S ? p[r][0] * xv[0] + p[r][1] * xv[1] + p[r][2] * xv[2] + p[r][3] * xv[3] : 0.f;
    }
    if (r0 < OC && k0 < S) {
#pragma unroll
        for (int r = 0; r < RB; ++r) p[r] = *reinterpret_cast<const f32x4*>(w2 + (size_t)min(r0 + r, OC - 1) * S + k0);
    }
    if (r0 < S) {
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            const float v = wave_sum_dpp(acc[r]) + __shfl(bv1, r, 64);
            if (lane == 0 && r0 + r < S) hid[r0 + r] = v > 0.f ? v : 0.f;
        }
    }
    __syncthreads();
    if (r0 < OC) {
        const f32x4 xv = k0 < S ? *reinterpret_cast<const f32x4*>(hid + k0) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < RB; ++r) acc[r] = k0 < S ? p[r][0] * xv[0] + p[r][1] * xv[1] + p[r][2] * xv[2] + p[r][3] * xv[3] : 0.f;
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            const float v = wave_sum_dpp(acc[r]) + __shfl(bv2, r, 64);
            if (lane == 0 && r0 + r < OC) { yo[r0 + r] = v; if (yhat_dbg) yhat_dbg[((size_t)b * T + t) * OC + r0 + r] = v; }
        }
    }
    __syncthreads();
    if (tid == 0) {
        float best = -INFINITY; int arg = 0;
        for (int k = 0; k < K; ++k) {
            float v = yo[k] - logf(-logf(us[k]));
            if (v > best) { best = v; arg = k; }
        }
        const float m = yo[K + arg], ls = fmaxf(yo[2 * K + arg], log_scale_min), u = us[K];
        float x = m + expf(ls) * (logf(u) - logf(1.f - u));
        out[(size_t)b * T + t] = fminf(fmaxf(x, -1.f), 1.f);
    }
}

// ---- the head as three row-parallel launches -------------------------------------------------------------------------------------
// wn_head_fused_kernel runs one block per stream: each of the 8 blocks pulls the 0.5 MB of head weights through ONE compute unit (25 us per
// time step, rocprofv3).  Spread over the rows instead -- a wave per row, every weight row read once for all streams, as the stages do:
//   rows kernel, mode 0: skips <- relu((skips + Ws z + bs) sqrt(.5))   (the last layer's skip rows; in place)
//   rows kernel, mode 1: hid   <- relu(W1 skips + b1)                   (hid lives in the z buffer the last stage did not write)
//   wn_head_sample_kernel: logits of stream b = W2 hid_b + b2 and the mixture-of-logistics sample (mixture.py:125-153, injected uniforms)
template <int NB>
__global__ __launch_bounds__(256) void wn_head_rows_kernel(const float* __restrict__ w, const float* __restrict__ bias, const float* __restrict__ x, int K,
                                                           float* __restrict__ out, int nrows, int mode, int first_skip) {
    WN_STRICT_FP
    const int o = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (o >= nrows) return;
    float acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[b] = 0.f;
    float pre = 0.f;
    if (mode == 0 && !first_skip && lane < NB) pre = out[(size_t)lane * nrows + o];
    const float bv = bias[o];
    for (int k = lane * 4; k < K; k += 256) {
        const f32x4 wv = *reinterpret_cast<const f32x4*>(w + (size_t)o * K + k);
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const f32x4 xv = *reinterpret_cast<const f32x4*>(x + (size_t)b * K + k);
            acc[b] += xv[0] * wv[0] + xv[1] * wv[1] + xv[2] * wv[2] + xv[3] * wv[3];
        }
    }
    const float r5 = 0.70710678118654752f;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const float v = wave_sum_dpp(acc[b]) + bv;
        const float p = __shfl(pre, b, 64);
        if (lane == 0) {
            const float y = mode == 0 ? (first_skip ? v : (p + v) * r5) : v;
            out[(size_t)b * nrows + o] = y > 0.f ? y : 0.f;
        }
    }
}

__global__ __launch_bounds__(256) void wn_head_sample_kernel(const float* __restrict__ hid, const float* __restrict__ w2, const float* __restrict__ b2,
                                                             const float* __restrict__ u1, const float* __restrict__ u2, float* __restrict__ out,
                                                             float* __restrict__ yhat_dbg, const int* __restrict__ step, int t_arg, int S, int OC, int T,
                                                             float log_scale_min) {
    __shared__ float yo[256];
    const int b = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int t = t_arg >= 0 ? t_arg : *step - 1;
    const int K3 = OC / 3;
    for (int o = wave; o < OC; o += 4) {
        float acc = 0.f;
        for (int k = lane * 4; k < S; k += 256) {
            const f32x4 wv = *reinterpret_cast<const f32x4*>(w2 + (size_t)o * S + k);
            const f32x4 xv = *reinterpret_cast<const f32x4*>(hid + (size_t)b * S + k);
            acc += xv[0] * wv[0] + xv[1] * wv[1] + xv[2] * wv[2] + xv[3] * wv[3];
        }
        const float v = wave_sum_dpp(acc) + b2[o];
        if (lane == 0) { yo[o] = v; if (yhat_dbg) yhat_dbg[((size_t)b * T + t) * OC + o] = v; }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float best = -INFINITY; int arg = 0;
        for (int k = 0; k < K3; ++k) {
            const float v = yo[k] - logf(-logf(u1[((size_t)b * T + t) * K3 + k]));
            if (v > best) { best = v; arg = k; }
        }
        const float m = yo[K3 + arg], ls = fmaxf(yo[2 * K3 + arg], log_scale_min), u = u2[(size_t)b * T + t];
        const float x = m + expf(ls) * (logf(u) - logf(1.f - u));
        out[(size_t)b * T + t] = fminf(fmaxf(x, -1.f), 1.f);
    }
}

// ---- categorical network: first conv, head rows, softmax + draw ---------------------------------------------------------------------------
// First conv, a wave per output channel c, every weight row read once for all streams.  Dense form: lane holds 4 of the K <= 256 columns, the
// wave sum has a fixed order.  Class form: lane b copies one element for stream b (skipped when `dense_only`: the fused stage 0 gathers itself).
template <int NB>
__global__ __launch_bounds__(256) void wn_cat_first_kernel(const WnCatIn in, const float* __restrict__ bias, float* __restrict__ ring, int ring_len,
                                                           const int* __restrict__ step, int t_arg, int C, int dense_only) {
    WN_STRICT_FP
    const int t = t_arg >= 0 ? t_arg : *step - 1;
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (c >= C) return;
    const int slot = t % ring_len;
    if (wn_cat_class_form<NB>(in, t)) {
        if (!dense_only && lane < NB) ring[((size_t)lane * ring_len + slot) * C + c] = in.w_t[(size_t)wn_cat_class(in, t, lane) * C + c] + bias[c];
        return;
    }
    const float bv = bias[c];
    float acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[b] = 0.f;
    for (int k = lane * 4; k < in.K; k += 256) {
        const f32x4 wv = *reinterpret_cast<const f32x4*>(in.w + (size_t)c * in.K + k);
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            if (in.forced != nullptr && wn_cat_class_form_of(in, t, b)) continue;      // a class stream in a mixed step: gathered below
            const f32x4 xv = *reinterpret_cast<const f32x4*>(wn_cat_row(in, t, b) + k);
            acc[b] += xv[0] * wv[0] + xv[1] * wv[1] + xv[2] * wv[2] + xv[3] * wv[3];
        }
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        float v = wave_sum_dpp(acc[b]);
        if (in.forced != nullptr && wn_cat_class_form_of(in, t, b)) v = in.w_t[(size_t)wn_cat_class(in, t, b) * C + c];
        if (lane == 0) ring[((size_t)b * ring_len + slot) * C + c] = v + bv;
    }
}

// a 1x1 layer of the head over all streams: out[b][o] = act(w[o] . relu(x[b]) + bias[o]); a wave per row o (wavenet.py:133-138: ReLU, 1x1, ReLU, 1x1)
template <int NB>
__global__ __launch_bounds__(256) void wn_cat_rows_kernel(const float* __restrict__ w, const float* __restrict__ bias, const float* __restrict__ x, int K,
                                                          float* __restrict__ out, int nrows, int relu_out) {
    WN_STRICT_FP
    const int o = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (o >= nrows) return;
    const float bv = bias[o];
    float acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[b] = 0.f;
    for (int k = lane * 4; k < K; k += 256) {
        const f32x4 wv = *reinterpret_cast<const f32x4*>(w + (size_t)o * K + k);
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const f32x4 xv = *reinterpret_cast<const f32x4*>(x + (size_t)b * K + k);
            acc[b] += fmaxf(xv[0], 0.f) * wv[0] + fmaxf(xv[1], 0.f) * wv[1] + fmaxf(xv[2], 0.f) * wv[2] + fmaxf(xv[3], 0.f) * wv[3];
        }
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const float v = wave_sum_dpp(acc[b]) + bv;
        if (lane == 0) out[(size_t)b * nrows + o] = relu_out ? fmaxf(v, 0.f) : v;
    }
}

// softmax over the K <= 256 logits of stream b = blockIdx.x (thread = class) and the categorical draw (wavenet.py:351-356).
//   softmax: p = exp(x - max) / sum, fp32 (F.softmax)
//   draw:    np.random.choice(K, p) from one uniform u: cdf = cumsum(p) (numpy: in fp64) / cdf[K - 1]; class = #{k: cdf[k] <= u}
//            (searchsorted side = "right"), at most K - 1.  The prefix sum is a wave64 scan plus a carry over the four waves added in wave order.
__global__ __launch_bounds__(256) void wn_cat_sample_kernel(const float* __restrict__ logits, const float* __restrict__ u, int* __restrict__ classes,
                                                            float* __restrict__ rows, const int* __restrict__ step, int t_arg, int K, int T,
                                                            int softmax, int quantize) {
    __shared__ float red[4];
    __shared__ double carry[4];
    __shared__ int cnt[4];
    const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int t = t_arg >= 0 ? t_arg : *step - 1;
    const bool live = tid < K;
    const float x = live ? logits[(size_t)b * K + tid] : -INFINITY;
    const float uu = quantize ? u[(size_t)b * T + t] : 0.f;
    float* row = rows ? rows + ((size_t)b * T + t) * K : nullptr;
    if (!softmax) {
        if (row && live) row[tid] = x;
        return;
    }
    float m = x;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if (lane == 0) red[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    const float e = live ? expf(x - m) : 0.f;
    const float p = e / block_sum(e, red);                          // block_sum's first barrier also fences the reads of red above
    if (!quantize) {
        if (row && live) row[tid] = p;
        return;
    }
    double v = (double)p;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double n = __shfl_up(v, o, 64);
        if (lane >= o) v += n;
    }
    if (lane == 63) carry[wave] = v;
    __syncthreads();
    double pre = 0.0;
    for (int w = 0; w < wave; ++w) pre += carry[w];
    const double total = ((carry[0] + carry[1]) + carry[2]) + carry[3];
    const double cdf = (pre + v) / total;
    const unsigned long long below = __ballot(live && cdf <= (double)uu);
    if (lane == 0) cnt[wave] = __popcll(below);
    __syncthreads();
    const int cls = min(cnt[0] + cnt[1] + cnt[2] + cnt[3], K - 1);
    if (tid == 0) classes[(size_t)b * T + t] = cls;
    if (row && live) row[tid] = tid == cls ? 1.f : 0.f;             // wavenet.py:355-356
}

__global__ __launch_bounds__(256) void mulaw_decode_kernel(const int* __restrict__ cls, float* __restrict__ out, long n, float mu) {
    const float l1p = log1pf(mu);
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256L) {
        const float y = 2.f * (float)cls[i] / mu - 1.f;
        const float mag = expm1f(fabsf(y) * l1p) / mu;              // ((1 + mu)^|y| - 1) / mu
        out[i] = y < 0.f ? -mag : mag;
    }
}

WnCatIn wn_cat_in(const viai_wn_synth* s, const unsigned char* forced) {
    WnCatIn in{};
    in.forced = forced;
    in.w_t = s->w_first_t; in.w = s->w_first; in.test_classes = s->test_classes; in.test_rows = s->test_inputs; in.init_rows = s->init_rows;
    in.classes = s->classes; in.rows = s->yhat_dbg; in.n_test = s->n_test; in.init_class = s->init_class; in.quantize = s->cat_quantize;
    in.K = s->out_ch; in.T = s->T;
    return in;
}

// host copy of wn_cat_class_form; t < 0 (time index on the device): "may a dense step occur at all".  With a mask of forced steps, which lives
// in device memory, the host can only say whether a step MAY be dense: a forced one (dense test rows), a fed-back one (no quantize) or a
// free first step from init_rows.  A launch this lets through for a step that turns out to be all classes returns at once.
bool wn_cat_dense_at(const viai_wn_synth* s, int t, const unsigned char* forced) {
    if (forced != nullptr) return s->test_classes == nullptr || !s->cat_quantize || (t <= 0 && s->init_rows != nullptr);
    if (t < 0) return (s->n_test > 0 && s->test_classes == nullptr) || !s->cat_quantize || (s->n_test == 0 && s->init_rows != nullptr);
    if (t < s->n_test) return s->test_classes == nullptr;
    if (t > 0) return !s->cat_quantize;
    return s->init_rows != nullptr;
}

// the output end of a categorical time step: the head's two 1x1 layers over all streams (hidden layer and logits in the scratch `out`), then
// softmax + draw, a block per stream.  `skips` holds the finished skip sum (the ReLU in front of W1 is applied on the read).
template <int NB>
void wn_cat_head(const viai_wn_synth* s, int t_arg, hipStream_t st) {
    const int S = s->S, K = s->out_ch;
    float* hid = s->out;
    float* logits = s->out + (size_t)s->B * S;
    VIAI_LAUNCH(wn_cat_rows_kernel<NB>, dim3((S + 3) / 4), dim3(256), 0, st, s->w_l1, s->b_l1, (const float*)s->skips, S, hid, S, 1);
    VIAI_LAUNCH(wn_cat_rows_kernel<NB>, dim3((K + 3) / 4), dim3(256), 0, st, s->w_l2, s->b_l2, (const float*)hid, S, logits, K, 0);
    VIAI_LAUNCH(wn_cat_sample_kernel, dim3(s->B), dim3(256), 0, st, (const float*)logits, s->u2, s->classes, s->yhat_dbg, s->step, t_arg, K, s->T,
                s->cat_softmax, s->cat_quantize);
}

bool wn_fused_ok(const viai_wn_synth* s) {
    if (!s->fused || s->z2 == nullptr) return false;
    if (s->S > 256 || s->out_ch > 256 || s->G / 2 > 256) return false;
    for (int l = 0; l < s->n_layers; ++l) if (s->layers[l].w_stage == nullptr || s->layers[l].b_stage == nullptr) return false;
    return true;
}

template <int NB>
int wn_step_fused_impl(const viai_wn_synth* s, int t_arg, hipStream_t st, const unsigned char* forced) {
    const int C = s->C, H = s->G / 2, S = s->S, n = s->n_layers;
    const viai_wn_layer* L = s->layers;
    if (t_arg < 0) VIAI_LAUNCH(wn_tick_kernel, dim3(1), dim3(1), 0, st, s->step);
    const bool cat = s->categorical != 0;
    if (cat && wn_cat_dense_at(s, t_arg, forced))
        VIAI_LAUNCH(wn_cat_first_kernel<NB>, dim3((C + 3) / 4), dim3(256), 0, st, wn_cat_in(s, forced), s->b_first, L[0].ring, L[0].ring_len, s->step, t_arg, C, 1);
    float* zb[2] = {s->z, s->z2};
    for (int l = 0; l < n; ++l) {
        WnStage a{};
        a.ring = L[l].ring; a.ring_len = L[l].ring_len; a.dil = L[l].dilation;
        a.w = L[l].w_stage; a.bias = L[l].b_stage; a.wc = L[l].w_c; a.cond = s->cond; a.gadd = L[l].g_add;
        a.z_out = zb[l & 1]; a.z_in = zb[(l & 1) ^ 1];
        a.w_first = s->w_first; a.b_first = s->b_first; a.test_inputs = s->test_inputs; a.n_test = s->n_test; a.out = s->out;
        a.ring_w = L[l].ring; a.skips = s->skips;
        if (l > 0) {
            a.ring_prev = L[l - 1].ring; a.prev_len = L[l - 1].ring_len;
            a.w_out = L[l - 1].w_out; a.b_out = L[l - 1].b_out; a.w_skip = L[l - 1].w_skip; a.b_skip = L[l - 1].b_skip;
            a.first_skip = (l == 1) ? 1 : 0;
        }
        a.step = s->step; a.t_arg = t_arg; a.l = l; a.C = C; a.H = H; a.S = S; a.cin = s->cin; a.T = s->T; a.B = s->B; a.forced = forced;
        const int nb = H + (l == 0 ? 1 : (C + S + 3) / 4);
        if (cat && l == 0) {
            a.cat = wn_cat_in(s, forced);
            VIAI_LAUNCH((wn_stage_kernel<NB, true>), dim3(nb), dim3(256), 0, st, a);
        } else {
            VIAI_LAUNCH(wn_stage_kernel<NB>, dim3(nb), dim3(256), 0, st, a);
        }
    }
    if (cat) {                                     // the last layer's skip rows (in place), then the categorical head
        VIAI_LAUNCH(wn_head_rows_kernel<NB>, dim3((S + 3) / 4), dim3(256), 0, st, L[n - 1].w_skip, L[n - 1].b_skip, (const float*)zb[(n - 1) & 1], H, s->skips, S, 0, n == 1 ? 1 : 0);
        wn_cat_head<NB>(s, t_arg, st);
        return viai_launch_status();
    }
    if (S <= H && s->out_ch <= 256) {
        float* zlast = zb[(n - 1) & 1];
        float* hid = zb[n & 1];                    // (B, S) fits the (B, H) buffer; the next time step's stage 0 overwrites it
        VIAI_LAUNCH(wn_head_rows_kernel<NB>, dim3((S + 3) / 4), dim3(256), 0, st, L[n - 1].w_skip, L[n - 1].b_skip, (const float*)zlast, H, s->skips, S, 0, n == 1 ? 1 : 0);
        VIAI_LAUNCH(wn_head_rows_kernel<NB>, dim3((S + 3) / 4), dim3(256), 0, st, s->w_l1, s->b_l1, (const float*)s->skips, S, hid, S, 1, 0);
        VIAI_LAUNCH(wn_head_sample_kernel, dim3(s->B), dim3(256), 0, st, (const float*)hid, s->w_l2, s->b_l2, s->u1, s->u2, s->out, s->yhat_dbg, s->step, t_arg, S,
                    s->out_ch, s->T, s->log_scale_min);
        return viai_launch_status();
    }
    VIAI_LAUNCH(wn_head_fused_kernel, dim3(s->B), dim3(1024), (2 * S + ((s->out_ch + 3) & ~3) + s->out_ch / 3 + 1) * sizeof(float), st,
                s->skips, zb[(n - 1) & 1], L[n - 1].w_skip, L[n - 1].b_skip, n == 1 ? 1 : 0, H, s->w_l1, s->b_l1, s->w_l2, s->b_l2, s->u1, s->u2,
                s->out, s->yhat_dbg, s->step, t_arg, S, s->out_ch, s->T, s->log_scale_min);
    return viai_launch_status();
}

template <int NB>
int wn_step_impl(const viai_wn_synth* s, int t_arg, hipStream_t st, const unsigned char* forced) {
    const int C = s->C, H = s->G / 2, S = s->S;
    const viai_wn_layer* L = s->layers;
    if (s->categorical) {                          // several blocks: the time index is advanced by a launch of its own, as in the fused form
        if (t_arg < 0) VIAI_LAUNCH(wn_tick_kernel, dim3(1), dim3(1), 0, st, s->step);
        VIAI_LAUNCH(wn_cat_first_kernel<NB>, dim3((C + 3) / 4), dim3(256), 0, st, wn_cat_in(s, forced), s->b_first, L[0].ring, L[0].ring_len, s->step, t_arg, C, 0);
    } else
    VIAI_LAUNCH(wn_first_kernel, dim3(1), dim3(256), 0, st, s->w_first, s->b_first, s->test_inputs, s->n_test, s->out,
                L[0].ring, L[0].ring_len, s->step, t_arg, s->B, C, s->T, forced);
    for (int l = 0; l < s->n_layers; ++l) {
        VIAI_LAUNCH(wn_gate_kernel<NB>, dim3(H), dim3(256), 0, st, L[l].ring, L[l].ring_len, L[l].dilation, L[l].w_conv, L[l].b_conv,
                    L[l].w_c, L[l].b_c, s->cond, L[l].g_add, s->z, s->step, t_arg, C, H, s->cin, s->T);
        const bool last = (l == s->n_layers - 1);
        VIAI_LAUNCH(wn_out_kernel<NB>, dim3((C + S + 3) / 4), dim3(256), 0, st, s->z, L[l].w_out, L[l].b_out, L[l].w_skip, L[l].b_skip,
                    L[l].ring, L[l].ring_len, last ? (float*)nullptr : L[l + 1].ring, last ? 1 : L[l + 1].ring_len, s->skips, l == 0 ? 1 : 0,
                    s->step, t_arg, C, H, S);
    }
    if (s->categorical) {
        wn_cat_head<NB>(s, t_arg, st);
        return viai_launch_status();
    }
    if (S <= 256 && s->out_ch <= 256)
        VIAI_LAUNCH(wn_head_kernel, dim3(s->B), dim3(1024), (2 * S + ((s->out_ch + 3) & ~3) + s->out_ch / 3 + 1) * sizeof(float), st, s->skips, s->w_l1, s->b_l1, s->w_l2, s->b_l2,
                    s->u1, s->u2, s->out, s->yhat_dbg, s->step, t_arg, S, s->out_ch, s->T, s->log_scale_min);
    else
        VIAI_LAUNCH(wn_head_generic_kernel, dim3(s->B), dim3(256), (2 * S + s->out_ch) * sizeof(float), st, s->skips, s->w_l1, s->b_l1, s->w_l2, s->b_l2,
                    s->u1, s->u2, s->out, s->yhat_dbg, s->step, t_arg, S, s->out_ch, s->T, s->log_scale_min);
    return viai_launch_status();
}

bool wn_valid(const viai_wn_synth* s) {
    if (!s || s->B < 1 || s->B > WN_MAXB || s->C % 4 != 0 || (s->G / 2) % 4 != 0 || s->cin % 4 != 0 || s->S % 4 != 0 || s->n_layers < 1) return false;
    if (!s->categorical) return s->out_ch % 3 == 0;             // [logit | mean | log_scale] x nr_mix: the mixture-of-logistics head only
    if (!viai_wn_categorical_ok(s)) return false;
    if (s->w_first == nullptr || s->w_first_t == nullptr || s->out == nullptr) return false;
    if (s->n_test > 0 && s->test_classes == nullptr && s->test_inputs == nullptr) return false;
    if (s->cat_quantize ? (s->classes == nullptr || s->u2 == nullptr) : s->yhat_dbg == nullptr) return false;
    return true;
}

int wn_step(const viai_wn_synth* s, int t_arg, hipStream_t st, const unsigned char* forced = nullptr) {
    if (wn_fused_ok(s)) {
        switch (s->B) {
        case 1: return wn_step_fused_impl<1>(s, t_arg, st, forced);
        case 2: return wn_step_fused_impl<2>(s, t_arg, st, forced);
        case 4: return wn_step_fused_impl<4>(s, t_arg, st, forced);
        case 8: return wn_step_fused_impl<8>(s, t_arg, st, forced);
        default: return (int)hipErrorInvalidValue;
        }
    }
    switch (s->B) {
    case 1: return wn_step_impl<1>(s, t_arg, st, forced);
    case 2: return wn_step_impl<2>(s, t_arg, st, forced);
    case 4: return wn_step_impl<4>(s, t_arg, st, forced);
    case 8: return wn_step_impl<8>(s, t_arg, st, forced);
    default: return (int)hipErrorInvalidValue;
    }
}

// a mask needs given inputs at all T steps (wn_valid has checked that the one-hot network has classes or rows where n_test > 0)
bool wn_forced_valid(const viai_wn_synth* s, const unsigned char* forced) {
    if (forced == nullptr) return true;
    return s->T >= 1 && s->n_test == s->T && (s->categorical || s->test_inputs != nullptr);
}

}  // namespace

extern "C" int viai_wn_categorical_ok(const viai_wn_synth* s) {
    if (!s || !s->categorical) return 0;
    if (s->B != 1 && s->B != 2 && s->B != 4 && s->B != 8) return 0;
    if (s->out_ch < 4 || s->out_ch > 256 || s->out_ch % 4 != 0) return 0;
    if (s->C < 4 || s->C % 4 != 0 || s->G < 8 || (s->G / 2) % 4 != 0 || s->cin % 4 != 0 || s->S < 4 || s->S % 4 != 0 || s->n_layers < 1) return 0;
    if (s->cat_quantize && !s->cat_softmax) return 0;           // logits are no probabilities (wavenet.py:351-354 raises there)
    if (s->init_class < 0 || s->init_class >= s->out_ch) return 0;
    return 1;
}

extern "C" int viai_mulaw_decode(const int* classes, float* out, long n, int mu, void* stream) {
    if (n < 0 || mu < 1) return (int)hipErrorInvalidValue;
    if (n == 0) return 0;
    VIAI_LAUNCH(mulaw_decode_kernel, dim3(ew_blocks(n)), dim3(256), 0, (hipStream_t)stream, classes, out, n, (float)mu);
    return viai_launch_status();
}

extern "C" int viai_wavenet_synth_step(const viai_wn_synth* s, void* stream) {
    if (!wn_valid(s)) return (int)hipErrorInvalidValue;
    return wn_step(s, -1, (hipStream_t)stream);
}

extern "C" int viai_wavenet_synth_run(const viai_wn_synth* s, int t0, int n_steps, void* stream) {
    if (!wn_valid(s) || t0 < 0 || n_steps < 0 || t0 + n_steps > s->T) return (int)hipErrorInvalidValue;
    for (int t = t0; t < t0 + n_steps; ++t) {
        const int e = wn_step(s, t, (hipStream_t)stream);
        if (e != 0) return e;
    }
    return 0;
}

extern "C" int viai_wavenet_synth_step_forced(const viai_wn_synth* s, const unsigned char* forced, void* stream) {
    if (!wn_valid(s) || !wn_forced_valid(s, forced)) return (int)hipErrorInvalidValue;
    return wn_step(s, -1, (hipStream_t)stream, forced);
}

extern "C" int viai_wavenet_synth_run_forced(const viai_wn_synth* s, const unsigned char* forced, int t0, int n_steps, void* stream) {
    if (!wn_valid(s) || !wn_forced_valid(s, forced) || t0 < 0 || n_steps < 0 || t0 + n_steps > s->T) return (int)hipErrorInvalidValue;
    for (int t = t0; t < t0 + n_steps; ++t) {
        const int e = wn_step(s, t, (hipStream_t)stream, forced);
        if (e != 0) return e;
    }
    return 0;
}
