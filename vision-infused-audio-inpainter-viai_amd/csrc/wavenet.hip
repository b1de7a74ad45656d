// WaveNet sample-by-sample synthesis, the chain forms (gfx950): the unfused, fused and one-hot (categorical) time step, each with or
// without a mask of forced steps, and the host dispatch behind viai_wavenet_synth_{step,run}[_forced].  Shared between kernels, once each:
// the time index (wn_time), the four-term dot (wn_dot4_strict / wn_dot4), the wave-per-row loop of the row-parallel head layers
// (wn_rows_dot) and the mixture-of-logistics draw of the four heads (viai_mol.h).  wn_gate_kernel / wn_out_kernel and the two halves of
// wn_stage_kernel, and wn_head_kernel and wn_head_fused_kernel, still hold the same stages twice: built from shared device functions the
// former ran slower and the latter changed its bits (profiles/wavenet_split_check.json).
// The training-side kernels (weight norm, GLU, losses, mu-law, ...) are wavenet_ops.hip, the pipelined form is wavenet_pipe.hip.
//
// Incremental synthesis (wavenet.py:237-364, conv.py:17-46).  One time step = first conv + per layer two
// GEMV-batch kernels (gate, then out/skip) + head (two 1x1 layers + MoL sample).  The time index lives in
// DEVICE memory (`step`), ring-buffer slots are derived from it inside the kernels, so every launch has static
// arguments and one step can be captured once into a hipGraph and replayed T times.
// Linearised weights: Wlin[g][j*C + ci] = w[g][ci][j] (conv.py:53-57), taps j = 0..2 read x[t-(2-j)*d].
#include "viai_common.h"
#include "viai_internal.h"
#include "viai_mol.h"

namespace {

constexpr int WN_MAXB = 8;

// A stream's arithmetic must not depend on how many streams travel with it: the kernels below are templates over the stream count NB, and with
// floating-point contraction left to the compiler each instantiation fused another subset of the products into its sums (it packs the streams
// pairwise: wn_out_kernel<1> had no fused multiply-add, <2> had), so stream b of a 4-stream run differed in the last bits from the 1-stream run
// on the same inputs.  WN_STRICT_FP, first statement of every NB-templated kernel, switches contraction off there: every product and sum is
// rounded on its own, in source order, whatever NB is.  The pragma is lexical: an inlined helper carries the setting of its OWN body, so every
// helper with arithmetic that those kernels call starts with it too, and the kernels without it (one block per stream: wn_first_kernel, the
// four MoL heads, wn_cat_sample_kernel) call only helpers without it.
#define WN_STRICT_FP _Pragma("clang fp contract(off)")

// ---- the shared pieces of a time step ---------------------------------------------------------------------------------------------------
// The time index of every kernel behind the first conv: by value (t_arg >= 0) or from device memory, which the first launch has advanced.
__device__ __forceinline__ int wn_time(const int* __restrict__ step, int t_arg) { return t_arg >= 0 ? t_arg : *step - 1; }

// Is the input of time step t of stream b given (teacher-forced)?  Without a mask: the common prefix t < n_test (wavenet.py:322-323).  With a
// mask `forced` (B, T) uint8 (viai_wavenet_synth_run_forced; the test inputs then cover all T steps, n_test == T): the mask's entry.
__device__ __forceinline__ bool wn_forced(const unsigned char* __restrict__ forced, int n_test, int T, int t, int b) {
    return forced != nullptr ? forced[(size_t)b * T + t] != 0 : t < n_test;
}

// x . w over one 16-byte chunk, x0 w0 + x1 w1 + x2 w2 + x3 w3 in this association.  The regimes, spelled out.  _strict, for the NB-templated
// kernels: every product and sum rounded.  The plain one, for the one-block-per-stream heads: contraction left to the compiler, as ever.
__device__ __forceinline__ float wn_dot4_strict(const f32x4 x, const f32x4 w) {
    WN_STRICT_FP
    return x[0] * w[0] + x[1] * w[1] + x[2] * w[2] + x[3] * w[3];
}
__device__ __forceinline__ float wn_dot4(const f32x4 x, const f32x4 w) { return x[0] * w[0] + x[1] * w[1] + x[2] * w[2] + x[3] * w[3]; }

// A wave per output row, every weight row read once for all NB streams: acc[b] = this lane's part of w_row . act(x[b]), act = ReLU if RELU_IN.
// wave_sum_dpp finishes the sum.
template <int NB, bool RELU_IN = false>
__device__ __forceinline__ void wn_rows_dot(const float* __restrict__ w_row, const float* __restrict__ x, size_t x_stride, int K, int lane,
                                            float (&acc)[NB]) {
    WN_STRICT_FP
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[b] = 0.f;
    for (int k = lane * 4; k < K; k += 256) {
        const f32x4 wv = *reinterpret_cast<const f32x4*>(w_row + k);
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            f32x4 xv = *reinterpret_cast<const f32x4*>(x + b * x_stride + k);
            if (RELU_IN) {
#pragma unroll
                for (int e = 0; e < 4; ++e) xv[e] = fmaxf(xv[e], 0.f);
            }
            acc[b] += wn_dot4_strict(xv, wv);
        }
    }
}

// ---- the plain form: first conv, gate and out/skip per layer, head --------------------------------------------------------------------------
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

// ---- the MoL head in one block of 16 waves per stream -----------------------------------------------------------------------------------
// wn_head_kernel and wn_head_fused_kernel keep their stages written out, each in its own text: they leave contraction to the compiler, and
// which products it fuses depends on how it packs neighbouring rows into two-float instructions.  Built from shared stage functions
// wn_head_fused_kernel packed its rows the way wn_head_kernel does and its sums changed in the last bits.
// head: relu -> W1 -> relu -> W2 -> MoL sample with injected uniforms -> out[b][t]; one block of 16 waves per stream.
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
    const int t = wn_time(step, t_arg);
    for (int k = tid; k < S; k += 1024) { float v = skips[(size_t)b * S + k]; xin[k] = v > 0.f ? v : 0.f; }
    if (tid < K) us[tid] = u1[((size_t)b * T + t) * K + tid];
    if (tid == K) us[K] = u2[(size_t)b * T + t];
    __syncthreads();
    // one 16-row batch: acc[r] = row (r0 + r) . x with the row slices already in registers (S <= 256: one 16-byte slice per lane)
    auto batch = [&](const float* __restrict__, const f32x4 (&pre)[RB], const float* x, int, float (&acc)[RB]) {
        const f32x4 xv = k0 < S ? *reinterpret_cast<const f32x4*>(x + k0) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < RB; ++r) acc[r] = k0 < S ? wn_dot4(pre[r], xv) : 0.f;
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
    if (tid == 0) out[(size_t)b * T + t] = viai_mol_draw(yo, us, us[K], K, log_scale_min);
}

// any S / out_ch: a row per thread (the first version of the head)
__global__ __launch_bounds__(256) void wn_head_generic_kernel(const float* __restrict__ skips, const float* __restrict__ w1, const float* __restrict__ b1,
                                                              const float* __restrict__ w2, const float* __restrict__ b2, const float* __restrict__ u1,
                                                              const float* __restrict__ u2, float* __restrict__ out, float* __restrict__ yhat_dbg,
                                                              const int* __restrict__ step, int t_arg, int S, int OC, int T, float log_scale_min) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* xin = sm; float* hid = sm + S; float* yo = sm + 2 * S;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int t = wn_time(step, t_arg);
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
    const int K = OC / 3;
    if (tid == 0) out[(size_t)b * T + t] = viai_mol_draw(yo, u1 + ((size_t)b * T + t) * K, u2[(size_t)b * T + t], K, log_scale_min);
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
    const int t = wn_time(step, t_arg);
    if (tid < K) us[tid] = u1[((size_t)b * T + t) * K + tid];
    if (tid == K) us[K] = u2[(size_t)b * T + t];
    float acc[RB];
    const float r5 = 0.70710678118654752f;
    if (r0 < S) {
        const f32x4 zv = k0 < H ? *reinterpret_cast<const f32x4*>(z + (size_t)b * H + k0) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < RB; ++r) acc[r] = k0 < H ? wn_dot4(p[r], zv) : 0.f;
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
        for (int r = 0; r < RB; ++r) acc[r] = k0 < S ? wn_dot4(p[r], xv) : 0.f;
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
        for (int r = 0; r < RB; ++r) acc[r] = k0 < S ? wn_dot4(p[r], xv) : 0.f;
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            const float v = wave_sum_dpp(acc[r]) + __shfl(bv2, r, 64);
            if (lane == 0 && r0 + r < OC) { yo[r0 + r] = v; if (yhat_dbg) yhat_dbg[((size_t)b * T + t) * OC + r0 + r] = v; }
        }
    }
    __syncthreads();
    if (tid == 0) out[(size_t)b * T + t] = viai_mol_draw(yo, us, us[K], K, log_scale_min);
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
    float pre = 0.f;
    if (mode == 0 && !first_skip && lane < NB) pre = out[(size_t)lane * nrows + o];
    const float bv = bias[o];
    float acc[NB];
    wn_rows_dot<NB>(w + (size_t)o * K, x, (size_t)K, K, lane, acc);
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
    const int t = wn_time(step, t_arg);
    const int K3 = OC / 3;
    for (int o = wave; o < OC; o += 4) {
        float acc = 0.f;
        for (int k = lane * 4; k < S; k += 256)
            acc += wn_dot4(*reinterpret_cast<const f32x4*>(hid + (size_t)b * S + k), *reinterpret_cast<const f32x4*>(w2 + (size_t)o * S + k));
        const float v = wave_sum_dpp(acc) + b2[o];
        if (lane == 0) { yo[o] = v; if (yhat_dbg) yhat_dbg[((size_t)b * T + t) * OC + o] = v; }
    }
    __syncthreads();
    if (threadIdx.x == 0) out[(size_t)b * T + t] = viai_mol_draw(yo, u1 + ((size_t)b * T + t) * K3, u2[(size_t)b * T + t], K3, log_scale_min);
}

// ---- categorical network: first conv, head rows, softmax + draw ---------------------------------------------------------------------------
// First conv, a wave per output channel c, every weight row read once for all streams.  Dense form: lane holds 4 of the K <= 256 columns, the
// wave sum has a fixed order.  Class form: lane b copies one element for stream b (skipped when `dense_only`: the fused stage 0 gathers itself).
// The dense loop is wn_rows_dot's with a row pointer and a skip condition per stream; it stays written out here.
template <int NB>
__global__ __launch_bounds__(256) void wn_cat_first_kernel(const WnCatIn in, const float* __restrict__ bias, float* __restrict__ ring, int ring_len,
                                                           const int* __restrict__ step, int t_arg, int C, int dense_only) {
    WN_STRICT_FP
    const int t = wn_time(step, t_arg);
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
            acc[b] += wn_dot4_strict(*reinterpret_cast<const f32x4*>(wn_cat_row(in, t, b) + k), wv);
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
    wn_rows_dot<NB, true>(w + (size_t)o * K, x, (size_t)K, K, lane, acc);
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
    const int t = wn_time(step, t_arg);
    const bool live = tid < K;
    const float x = live ? logits[(size_t)b * K + tid] : -INFINITY;
    const float uu = quantize ? u[(size_t)b * T + t] : 0.f;
    float* row = rows ? rows + ((size_t)b * T + t) * K : nullptr;
    if (!softmax) {
        if (row && live) row[tid] = x;
        return;
    }
    float m = wave_max(x);
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

// ---- host: one time step as launches --------------------------------------------------------------------------------------------------------
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

// dynamic LDS of wn_head_kernel / wn_head_fused_kernel (WnHeadLds)
size_t wn_head_lds_bytes(const viai_wn_synth* s) { return (2 * s->S + ((s->out_ch + 3) & ~3) + s->out_ch / 3 + 1) * sizeof(float); }

// the argument of stage l: it writes z into zb[l & 1] and reads layer l - 1's from the other buffer
WnStage wn_stage_args(const viai_wn_synth* s, int l, float* const (&zb)[2], int t_arg, const unsigned char* forced) {
    const viai_wn_layer* L = s->layers;
    WnStage a{};
    if (s->categorical && l == 0) a.cat = wn_cat_in(s, forced);
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
    a.step = s->step; a.t_arg = t_arg; a.l = l; a.C = s->C; a.H = s->G / 2; a.S = s->S; a.cin = s->cin; a.T = s->T; a.B = s->B; a.forced = forced;
    return a;
}

template <int NB>
int wn_step_fused_impl(const viai_wn_synth* s, int t_arg, hipStream_t st, const unsigned char* forced) {
    const int C = s->C, H = s->G / 2, S = s->S, n = s->n_layers;
    const viai_wn_layer* L = s->layers;
    if (t_arg < 0) VIAI_LAUNCH(wn_tick_kernel, dim3(1), dim3(1), 0, st, s->step);
    const bool cat = s->categorical != 0;
    if (cat && wn_cat_dense_at(s, t_arg, forced))
        VIAI_LAUNCH(wn_cat_first_kernel<NB>, dim3((C + 3) / 4), dim3(256), 0, st, wn_cat_in(s, forced), s->b_first, L[0].ring, L[0].ring_len, s->step, t_arg, C, 1);
    float* const zb[2] = {s->z, s->z2};
    for (int l = 0; l < n; ++l) {
        const WnStage a = wn_stage_args(s, l, zb, t_arg, forced);
        const int nb = H + (l == 0 ? 1 : (C + S + 3) / 4);
        if (cat && l == 0) VIAI_LAUNCH((wn_stage_kernel<NB, true>), dim3(nb), dim3(256), 0, st, a);
        else VIAI_LAUNCH(wn_stage_kernel<NB>, dim3(nb), dim3(256), 0, st, a);
    }
    const float* zlast = zb[(n - 1) & 1];
    const int first = n == 1 ? 1 : 0;
    auto skip_rows = [&] {                         // the last layer's skip rows, in place
        VIAI_LAUNCH(wn_head_rows_kernel<NB>, dim3((S + 3) / 4), dim3(256), 0, st, L[n - 1].w_skip, L[n - 1].b_skip, zlast, H, s->skips, S, 0, first);
    };
    if (cat) {
        skip_rows();
        wn_cat_head<NB>(s, t_arg, st);
    } else if (S <= H && s->out_ch <= 256) {
        float* hid = zb[n & 1];                    // (B, S) fits the (B, H) buffer; the next time step's stage 0 overwrites it
        skip_rows();
        VIAI_LAUNCH(wn_head_rows_kernel<NB>, dim3((S + 3) / 4), dim3(256), 0, st, s->w_l1, s->b_l1, (const float*)s->skips, S, hid, S, 1, 0);
        VIAI_LAUNCH(wn_head_sample_kernel, dim3(s->B), dim3(256), 0, st, (const float*)hid, s->w_l2, s->b_l2, s->u1, s->u2, s->out, s->yhat_dbg, s->step, t_arg, S,
                    s->out_ch, s->T, s->log_scale_min);
    } else {
        VIAI_LAUNCH(wn_head_fused_kernel, dim3(s->B), dim3(1024), wn_head_lds_bytes(s), st, s->skips, zlast, L[n - 1].w_skip, L[n - 1].b_skip, first, H,
                    s->w_l1, s->b_l1, s->w_l2, s->b_l2, s->u1, s->u2, s->out, s->yhat_dbg, s->step, t_arg, S, s->out_ch, s->T, s->log_scale_min);
    }
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
        VIAI_LAUNCH(wn_head_kernel, dim3(s->B), dim3(1024), wn_head_lds_bytes(s), st, s->skips, s->w_l1, s->b_l1, s->w_l2, s->b_l2,
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

// a mask needs given inputs at all T steps (wn_valid has checked that the one-hot network has classes or rows where n_test > 0)
bool wn_forced_valid(const viai_wn_synth* s, const unsigned char* forced) {
    if (forced == nullptr) return true;
    return s->T >= 1 && s->n_test == s->T && (s->categorical || s->test_inputs != nullptr);
}

// the only switch over the stream counts the kernels are instantiated for: f(std::integral_constant<int, NB>)
template <class F>
int wn_for_streams(int B, F&& f) {
    switch (B) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 8: return f(std::integral_constant<int, 8>{});
    default: return (int)hipErrorInvalidValue;
    }
}

// what the four entry points do: time steps t0 .. t0 + n - 1 with the index passed by value, or (t0 = -1) the one step whose index is on the device
int wn_run(const viai_wn_synth* s, const unsigned char* forced, int t0, int n, void* stream) {
    if (!wn_valid(s) || !wn_forced_valid(s, forced) || (t0 >= 0 && (n < 0 || t0 + n > s->T))) return (int)hipErrorInvalidValue;
    const bool fused = wn_fused_ok(s);
    for (int t = t0; t < t0 + n; ++t) {
        const int e = wn_for_streams(s->B, [&](auto nb) {
            constexpr int NB = decltype(nb)::value;
            return fused ? wn_step_fused_impl<NB>(s, t, (hipStream_t)stream, forced) : wn_step_impl<NB>(s, t, (hipStream_t)stream, forced);
        });
        if (e != 0) return e;
    }
    return 0;
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

extern "C" int viai_wavenet_synth_step(const viai_wn_synth* s, void* stream) { return wn_run(s, nullptr, -1, 1, stream); }

extern "C" int viai_wavenet_synth_run(const viai_wn_synth* s, int t0, int n_steps, void* stream) {
    return t0 < 0 ? (int)hipErrorInvalidValue : wn_run(s, nullptr, t0, n_steps, stream);
}

extern "C" int viai_wavenet_synth_step_forced(const viai_wn_synth* s, const unsigned char* forced, void* stream) { return wn_run(s, forced, -1, 1, stream); }

extern "C" int viai_wavenet_synth_run_forced(const viai_wn_synth* s, const unsigned char* forced, int t0, int n_steps, void* stream) {
    return t0 < 0 ? (int)hipErrorInvalidValue : wn_run(s, forced, t0, n_steps, stream);
}
