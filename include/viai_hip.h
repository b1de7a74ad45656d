/* viai_hip.h — C ABI of libviai_hip.so, the MI355X (gfx950) kernel library for the
 * VIAI spectrogram-inpainting GAN hot path.
 *
 * The reference (Hangz-nju-cuhk/Vision-Infused-Audio-Inpainter-VIAI) has no FFI /
 * operator registry: its hot path is torch.nn calls inside nn.Modules (SURVEY.md
 * §8b).  Each entry point below therefore names the reference call site(s) whose
 * ATen dispatch it replaces (paths relative to the reference root).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller.  The library allocates no device memory and keeps no state BETWEEN
 *     calls that affects results.  What it does keep, per process: the VIAI_* environment switches (read once), the
 *     max-dynamic-LDS attribute of each kernel (set once), a per-thread first-error slot (cleared by every entry point), and the
 *     launch-plan log / plans (viai_plan_*: host memory and hipEvents owned by the plan, freed by viai_plan_destroy);
 *   - activations are fp32 NHWC: [N][H][W][C], C contiguous.  A (N,1,H,W) NCHW
 *     tensor is bit-identical to its NHWC form;
 *   - `stream` is a hipStream_t passed as void*; launches are asynchronous on it,
 *     the library never synchronises;
 *   - return value: 0 (hipSuccess) or a hipError_t / hipErrorInvalidValue code.
 *     Nothing throws across this boundary.
 *   - entry points may be called from several host threads on different streams (the launch-plan log is the exception: one
 *     recording at a time); one process per GPU under data parallelism.
 */
#ifndef VIAI_HIP_H
#define VIAI_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VIAI_ABI_VERSION 20

enum { VIAI_ACT_NONE = 0, VIAI_ACT_RELU = 1, VIAI_ACT_LRELU = 2, VIAI_ACT_SIGMOID = 3 };

int viai_abi_version(void);

/* ---------------------------------------------------------------- convolution
 * nn.Conv2d / stride-1 nn.ConvTranspose2d as used by
 *   MelEncoder            networks/Inpainting_Networks.py:55-63
 *   TransConvBlock        networks/New_Inpainting_Networks.py:24
 *   MelDecoder            networks/New_Inpainting_Networks.py:53-63
 *   MelDiscriminator      networks/Discriminator_Networks.py:17-33
 * `x2` (may be NULL) is a second input concatenated after x on the channel axis
 * (replaces torch.cat at New_Inpainting_Networks.py:81 without the copy).       */
typedef struct viai_conv2d {
    int N, IH, IW;       /* input batch / height / width                           */
    int C1, C2;          /* channels of x and of x2 (C2 = 0 when x2 == NULL)       */
    int Cout;
    int kh, kw, sh, sw, ph, pw;
    int transposed;      /* 0 = nn.Conv2d (weight [Cout][Cin][kh][kw]);
                            1 = nn.ConvTranspose2d, stride 1 (weight [Cin][Cout][kh][kw]) */
    int dh, dw;          /* dilation (0 or 1 = none); nn.Conv2d only.  WaveNet's dilated causal Conv1d
                            (wavenet_vocoder/modules.py:124-126) is kh = 1, kw = 3, dw = 2^i            */
    int ph2, pw2;        /* bottom / right padding; -1 = same as ph / pw (torch's symmetric padding).
                            pw = (k-1)*d, pw2 = 0 computes exactly the T causal outputs the reference keeps
                            after `x[:, :, :residual.size(-1)]` (modules.py:181)                          */
} viai_conv2d;

/* output extent (torch formulas) */
int viai_conv2d_out_hw(const viai_conv2d* c, int* OH, int* OW);
/* floats needed for one packed copy of the weights (forward or dgrad form).  The packed image is opaque:
 * fp32 [Cout][taps][Cin], or three bf16 planes (row-major or MFMA-fragment-major) for the bf16x3 kernels. */
size_t viai_conv2d_packed_floats(const viai_conv2d* c);
/* repack torch-layout weights for the forward / data-gradient kernels */
int viai_conv2d_pack_fwd(const viai_conv2d* c, const float* w, float* wp, void* stream);
int viai_conv2d_pack_dgrad(const viai_conv2d* c, const float* w, float* wp, void* stream);
/* Batched weight packing: every bf16x3 weight image of a model in one launch (the weights change once per optimizer
 * step; ~60 five-microsecond pack launches per step otherwise sit on the critical path).  viai_conv2d_pack_job fills
 * one job (frag: 0 = row-major bf16x3 planes, 1 = fragment-major bf16x3 planes, 2 = fp32 [n_out][tap][k_in]; returns 1
 * for the row-run image of the 7x7 image-input conv: pack that one with viai_conv2d_pack_fwd); the
 * caller sets blk0 to the running sum of nblk, uploads the array and launches it with viai_pack_jobs_run.      */
typedef struct viai_pack_job {
    const void* w; void* wp;
    int n_out, k_in, taps, frag;
    long s_no, s_ki;
    int blk0, nblk;
} viai_pack_job;
int viai_conv2d_pack_job(const viai_conv2d* c, int dgrad, const float* w, float* wp, viai_pack_job* job);
int viai_pack_jobs_run(const viai_pack_job* jobs_dev, int njobs, int total_blocks, void* stream);
/* BatchNorm partial-statistics geometry of the forward kernel: number of row
 * blocks and rows per block; stat_part holds 2*Cout*nblk floats.                */
int viai_conv2d_stat_geom(const viai_conv2d* c, int* nblk, int* rows_per_blk);
/* (ABI 9) Where the forward kernel works on 2-D output tiles and the map is not a whole number of them, the partial blocks are
 * tiles clipped at the map's edge (block = (n, tile row, tile column), row-major), not runs of rows_per_blk rows: tile_h x tile_w
 * is returned here (0, 0 otherwise) and the partials go to viai_bn_finalize_tiles instead of viai_bn_finalize.                    */
int viai_conv2d_stat_tiles(const viai_conv2d* c, int* tile_h, int* tile_w);
/* y = conv(x ++ x2, w) + bias [; act].  stat_part (optional) receives per-block
 * per-channel (mean, M2) of y for training-mode BatchNorm; act must be NONE then. */
int viai_conv2d_fwd(const viai_conv2d* c, const float* x, const float* x2, const float* wp_fwd,
                    const float* bias, float* y, float* stat_part, int act, void* stream);
/* The same with the magnitude of the input known.  The f16x2 kernels (two-term fp16 operand split) pre-scale the activation
 * operand by a power of two: with x_amax -- a DEVICE float >= max |x| (and |x2|), produced by viai_bn_act_fwd_amax /
 * viai_conv2d_cin1_bn_fwd / viai_absmax -- the scale is derived on the device and every magnitude is representable; with
 * x_amax = NULL (and in viai_conv2d_fwd) it is the static 16, right for normalised activations, and |x| beyond 65504 / 16 = 4094
 * saturates.  Kernels that do not split (fp32, bf16x3, the streaming kernels) ignore it.                                        */
int viai_conv2d_fwd_f16_ok(const viai_conv2d* c);      /* 1: the forward launch of this layer is an f16x2 kernel */
int viai_conv2d_fwd_amax(const viai_conv2d* c, const float* x, const float* x2, const float* wp_fwd,
                         const float* bias, float* y, float* stat_part, int act, const float* x_amax, void* stream);
/* amax = max(amax, max |x|) over n floats (x 16-byte aligned): the operand magnitude of a tensor this library did not produce;
 * *amax must hold 0 or an earlier maximum.  One streaming pass.                                                              */
int viai_absmax(const float* x, long n, float* amax, void* stream);
/* dx (++ dx2) = conv_backward_data(dy, w) */
int viai_conv2d_dgrad(const viai_conv2d* c, const float* dy, const float* wp_dgrad,
                      float* dx, float* dx2, void* stream);
/* f16x2 data gradient for the layers whose data gradient runs on the wide-tile kernel (viai_conv2d_dgrad_f16_ok): half the
 * MFMA work of the bf16x3 form.  fp16 has a narrow exponent range and gradients span many decades, so the kernel scales dy
 * by a power of two derived ON THE DEVICE from dy_amax = max |dy| (one float, written by viai_bn_act_bwd_amax).
 * Weights: viai_conv2d_pack_dgrad_f16 (or viai_conv2d_pack_job with dgrad = 2).                                        */
int viai_conv2d_dgrad_f16_ok(const viai_conv2d* c);
int viai_conv2d_pack_dgrad_f16(const viai_conv2d* c, const float* w, float* wp, void* stream);
int viai_conv2d_dgrad_f16(const viai_conv2d* c, const float* dy, const float* wp, float* dx, float* dx2,
                          const float* dy_amax, void* stream);
/* dw (torch layout) = conv_backward_weight(x ++ x2, dy); dw += if accumulate.
 * db (optional, [Cout]) = sum of dy.  ws: scratch of viai_conv2d_wgrad_ws_bytes. */
size_t viai_conv2d_wgrad_ws_bytes(const viai_conv2d* c);
int viai_conv2d_wgrad(const viai_conv2d* c, const float* x, const float* x2, const float* dy,
                      float* ws, float* dw, float* db, int accumulate, void* stream);
/* f16x2 form of the weight gradient (viai_conv2d_wgrad_f16_ok: layers with more than 32 channels on both sides): dy is
 * scaled on the device from dy_amax = max |dy| (viai_bn_act_bwd_amax), x from x_amax >= max |x|, |x2| (see
 * viai_conv2d_fwd_amax) or, with x_amax = NULL, by the static 16                                                        */
int viai_conv2d_wgrad_f16_ok(const viai_conv2d* c);
int viai_conv2d_wgrad_f16(const viai_conv2d* c, const float* x, const float* x2, const float* dy,
                          float* ws, float* dw, float* db, int accumulate, const float* dy_amax, const float* x_amax, void* stream);

/* Which kernel ran.  The convolution entry points above (and viai_conv2d_cin1_bn_fwd / _wgrad) choose between kernel families by
 * shape; this reports the family the LAST such call of the calling thread launched and how many conv-kernel launches it made
 * (a strided data gradient on the gather kernel is one launch per parity class).  The name ends in the arithmetic of the
 * kernel -- "_f16x2" (two-term fp16 split, 3 MFMA products per MAC), "_bf16x3" (three-term bf16 split, 6 products), "_f32"
 * (exact fp32 MFMA) -- or is "direct" for the Cin = 1 / Cout = 1 streaming kernels; bench.py prices each family against the
 * ceiling of that arithmetic.  buf receives the NUL-terminated name (truncated to cap); returns the launch count, 0 if none.
 * (measurement aid: no reference counterpart)                                                                             */
int viai_conv2d_last_kernel(char* buf, int cap);
/* (ABI 18) The same answer without a launch (host code only): the family name viai_conv2d_last_kernel would report after the launch of
 * this layer in direction `pass` (0 forward, 1 data gradient, 2 weight gradient) with operands of `form`, written to family
 * (NUL-terminated, truncated to cap); returns the number of conv-kernel launches, 0 with an empty name if the entry point would
 * refuse the call.  (Cin = 1 / Cout = 1 layers answer 1 x "direct" like the tag: the streaming kernels check strides and channel
 * counts of their own at the launch, after the tag is set.)  form: VIAI_FORM_F32 (viai_conv2d_fwd / _dgrad / _wgrad), VIAI_FORM_AMAX (the _amax / _f16 entry points),
 * VIAI_FORM_P16 (the _p16 entry points); for the weight gradient's P16 form add its flags: VIAI_FORM_P16 | (flags << 2).       */
#define VIAI_FORM_F32 0
#define VIAI_FORM_AMAX 1
#define VIAI_FORM_P16 2
int viai_conv2d_route(const viai_conv2d* c, int pass, int form, char* family, int cap);

/* generic weight repack used by the two pack entry points (exposed for tests):
 * wp[no][t][ki] = w[no*s_no + ki*s_ki + t]                                       */
int viai_pack_weight(const float* w, float* wp, int n_out, int k_in, int taps,
                     long s_no, long s_ki, void* stream);

/* ------------------------------------------------------------ batch-norm + act
 * nn.BatchNorm2d in training mode followed by LeakyReLU(0.2) / ReLU
 * (Inpainting_Networks.py:72-76, New_Inpainting_Networks.py:33-36,72-75,86,
 *  Discriminator_Networks.py:39-46).                                            */
/* merge block partials -> mean / invstd / (scale, shift); update running stats
 * (momentum, unbiased variance) and num_batches_tracked (int64, may be NULL).
 * Not for the partials of a viai_conv2d_fwd_p16 launch on a layer that reports VIAI_P16_OK_FWD_LIN: those are laid out for
 * viai_bn_finalize_lin below.                                                    */
int viai_bn_finalize(const float* stat_part, int nblk, int rows_per_blk, long M, int C,
                     const float* gamma, const float* beta, float* running_mean, float* running_var,
                     int64_t* num_batches_tracked, float momentum, float eps,
                     float* mean, float* invstd, float* scale, float* shift, void* stream);
/* (ABI 9) the same merge where block b = tile (n, ty, tx) of tile_h x tile_w output pixels clipped at the edge of the OH x OW map
 * (viai_conv2d_stat_tiles): N * ceil(OH / tile_h) * ceil(OW / tile_w) blocks of min(tile_h, OH - ty tile_h) * min(tile_w, OW - tx tile_w) rows */
/* (ABI 17) the finalize behind a pre-split forward on the linear-tile kernel (VIAI_P16_OK_FWD_LIN in viai_conv2d_p16_ok): its partials are per 128 consecutive pixels
 * or, for layers with one channel block (Cout 64 / 128 / 256), merged per persistent block inside the conv kernel -- the library applies the same rule here as at
 * the launch.  Replaces the nn.BatchNorm2d statistics of networks/ResNet.py:26-55 behind those convs; stat_part as sized by viai_conv2d_stat_geom. */
int viai_bn_finalize_lin(const float* stat_part, long M, int C,
                         const float* gamma, const float* beta, float* running_mean, float* running_var,
                         int64_t* nbt, float momentum, float eps,
                         float* mean, float* invstd, float* scale, float* shift, void* stream);
int viai_bn_finalize_tiles(const float* stat_part, int N, int OH, int OW, int tile_h, int tile_w, int C,
                           const float* gamma, const float* beta, float* running_mean, float* running_var,
                           int64_t* num_batches_tracked, float momentum, float eps,
                           float* mean, float* invstd, float* scale, float* shift, void* stream);
/* eval mode: (scale, shift) from the running statistics */
int viai_bn_eval_coeffs(int C, const float* gamma, const float* beta, const float* running_mean,
                        const float* running_var, float eps, float* mean, float* invstd,
                        float* scale, float* shift, void* stream);
/* z = act(y*scale[c] + shift[c]) */
int viai_bn_act_fwd(const float* y, const float* scale, const float* shift, float* z,
                    long M, int C, int act, float slope, void* stream);
/* the same, also reducing max |z| into the device float z_amax (zero-initialised by the caller; NULL = off): the operand
 * magnitude the f16x2 kernels that consume z are handed (viai_conv2d_fwd_amax, viai_conv2d_wgrad_f16)                   */
int viai_bn_act_fwd_amax(const float* y, const float* scale, const float* shift, float* z,
                         long M, int C, int act, float slope, float* z_amax, void* stream);
/* backward of the pair above (training-mode statistics):
 *   dgamma, dbeta (optional outputs) and dy.  part: scratch of 2*C*nblk floats,
 *   nblk from viai_bn_bwd_blocks(M, C).  `training` bit 0: 1 = batch statistics, 0 = eval-mode rule;
 *   bit 1: accumulate into dgamma/dbeta instead of overwriting them.               */
int viai_bn_bwd_blocks(long M, int C);
int viai_bn_act_bwd(const float* dz, const float* y, const float* mean, const float* invstd,
                    const float* scale, const float* shift, float* part, float* sums,
                    float* dgamma, float* dbeta, float* dy, long M, int C, int act, float slope,
                    int training, void* stream);
/* the same, and *amax (one float, zero-initialised by the caller) receives max |dy| */
int viai_bn_act_bwd_amax(const float* dz, const float* y, const float* mean, const float* invstd,
                         const float* scale, const float* shift, float* part, float* sums,
                         float* dgamma, float* dbeta, float* dy, long M, int C, int act, float slope,
                         int training, float* amax, void* stream);
/* elementwise activation backward for layers without BN (sigmoid heads):
 * dx = dz * act'(.) expressed through the activation OUTPUT z                    */
int viai_act_bwd_from_output(const float* dz, const float* z, float* dx, long n, int act,
                             float slope, void* stream);
/* (ABI 15) the same on a gradient that arrives as two addends: dx = (dz + dz2) * act'(.); n a multiple of 4.  The residual join of
 * networks/ResNet.py:46-53: d(out) = conv1's data gradient + the next join's residual gradient, summed where the ReLU mask is applied */
int viai_add_act_bwd_from_output(const float* dz, const float* dz2, const float* z, float* dx, long n, int act,
                                 float slope, void* stream);

/* ------------------------------------------------------------------ resampling
 * F.interpolate(mode='bilinear', align_corners=True)  New_Inpainting_Networks.py:78,83 */
int viai_bilinear_ac_fwd(const float* x, float* y, int N, int IH, int IW, int OH, int OW, int C, void* stream);
int viai_bilinear_ac_bwd(const float* dy, float* dx, int N, int IH, int IW, int OH, int OW, int C, void* stream);
/* BatchNorm apply + activation + the resize in one pass: out = interpolate(act(scale * y + shift), size=(OH, OW), mode="bilinear",
 * align_corners=True) -- the last layer of each decoder block and the F.interpolate behind it (New_Inpainting_Networks.py:76-83); the
 * post-activation map is not stored.  act: none / ReLU / LeakyReLU; C / 4 a power of two <= 256; N * OH * OW < 2^24.  *z_amax (optional,
 * zero-initialised): max |act(..)| over the taps read, the whole map's when the resize does not shrink it (ABI 12)                      */
int viai_bn_act_bilinear_fwd_amax(const float* y, const float* scale, const float* shift, float* out, int N, int IH, int IW,
                                  int OH, int OW, int C, int act, float slope, float* z_amax, void* stream);
/* nn.AvgPool2d((3,1)) on the bottleneck  Inpainting_Networks.py:65,77 (floor mode) */
int viai_avgpool_h_fwd(const float* x, float* y, int N, int IH, int W, int C, int k, void* stream);
int viai_avgpool_h_bwd(const float* dy, float* dx, int N, int IH, int W, int C, int k, void* stream);

/* ResNet-18 visual branch (networks/Image_Embedding.py:13-71, networks/ResNet.py:26-55).
 * For 1 < C1 <= 4 (conv1 on RGB / flow frames) the conv entry points expect x stored with channel stride 4
 * (zero padded): viai_nchw_to_nhwc4 produces that layout from the loader's NCHW frames.                */
int viai_nchw_to_nhwc4(const float* x, float* y, long N, int C, long HW, void* stream);
/* (ABI 15) the same, and max |x| into *amax (one zero-initialised float): the operand scale of the stem conv's f16x2 kernels */
int viai_nchw_to_nhwc4_amax(const float* x, float* y, long N, int C, long HW, float* amax, void* stream);
/* nn.MaxPool2d(k, s, p); idx: one byte per output element (window argmax) kept for the backward */
int viai_maxpool_fwd(const float* x, float* y, unsigned char* idx, int N, int IH, int IW, int C, int k, int s, int p, void* stream);
int viai_maxpool_bwd(const float* dy, const unsigned char* idx, float* dx, int N, int IH, int IW, int C, int k, int s, int p, void* stream);
/* nn.AvgPool2d(7) on a 7x7 map: mean over the P = H*W positions */
int viai_avgpool_hw_fwd(const float* x, float* y, int N, int P, int C, void* stream);
int viai_avgpool_hw_bwd(const float* dy, float* dx, int N, int P, int C, void* stream);
/* F.avg_pool2d(x, k, s, p, count_include_pad=False): input pyramid of the multi-scale discriminator (cfg 4) */
int viai_avgpool2d_fwd(const float* x, float* y, int N, int IH, int IW, int C, int k, int s, int p, void* stream);
int viai_avgpool2d_bwd(const float* dy, float* dx, int N, int IH, int IW, int C, int k, int s, int p, void* stream);
/* BasicBlock join: out = relu(a + b); backward d = g * (out > 0) (same for both addends) */
int viai_add_relu_fwd(const float* a, const float* b, float* out, long n, void* stream);
/* (ABI 10) the BatchNorm-apply pass fused with what follows it in the ResNet branch (networks/ResNet.py:43-55, Image_Embedding.py:20-23):
 *   viai_bn_add_act_fwd_amax : z = act(scale*y + shift + res)            bn2 -> += identity -> ReLU of a BasicBlock in one pass
 *   viai_bn_act_maxpool_fwd  : out = maxpool_{k,s,p}(act(scale*y + shift)) + argmax bytes; the stem's post-activation map is never stored
 *   viai_bn_act_pool_bwd_amax: viai_bn_act_bwd_amax with the gradient of that map gathered from (dpool, idx) where it is loaded
 * act = VIAI_ACT_RELU or VIAI_ACT_NONE.                                                                                            */
int viai_bn_add_act_fwd_amax(const float* y, const float* scale, const float* shift, const float* res, float* z,
                             long M, int C, int act, float slope, float* z_amax, void* stream);
int viai_bn_act_maxpool_fwd(const float* y, const float* scale, const float* shift, float* out, unsigned char* idx,
                            int N, int IH, int IW, int C, int k, int s, int p, int act, float slope, float* out_amax, void* stream);
int viai_bn_act_pool_bwd_amax(const float* dpool, const unsigned char* idx, int N, int IH, int IW, int k, int s, int p,
                              const float* y, const float* mean, const float* invstd, const float* scale, const float* shift,
                              float* part, float* sums, float* dgamma, float* dbeta, float* dy, int C, int act, float slope,
                              int training, float* amax, void* stream);
/* (ABI 15) the pooled gradient as two addends, summed where it is loaded (dpool2 may be NULL) */
int viai_bn_act_pool_bwd_amax2(const float* dpool, const float* dpool2, const unsigned char* idx, int N, int IH, int IW, int k, int s, int p,
                               const float* y, const float* mean, const float* invstd, const float* scale, const float* shift,
                               float* part, float* sums, float* dgamma, float* dbeta, float* dy, int C, int act, float slope,
                               int training, float* amax, void* stream);
int viai_relu_bwd(const float* g, const float* out, float* d, long n, void* stream);

/* ----------------------------------------------------------------------- losses
 * GANLoss = BCELoss / MSELoss against an expanded scalar label (loss_functions.py:79-104);
 * L1 is the `loss_mel_L1_item` metric (train_whole_sync.py:111).  Each forward
 * writes ONE float (mean reduction) to `loss`; `part` is scratch of
 * viai_reduce_blocks(n) floats.  Backward multiplies by the scalar *gscale
 * (device pointer; e.g. d(total)/d(loss)).                                       */
int viai_reduce_blocks(long n);
int viai_bce_fwd(const float* p, float target, long n, float* part, float* loss, void* stream);
int viai_bce_bwd(const float* p, float target, long n, const float* gscale, float* dp, void* stream);
int viai_mse_fwd(const float* p, float target, long n, float* part, float* loss, void* stream);
int viai_mse_bwd(const float* p, float target, long n, const float* gscale, float* dp, void* stream);
int viai_l1_fwd(const float* a, const float* b, long n, float* part, float* loss, void* stream);
int viai_l1_bwd(const float* a, const float* b, long n, const float* gscale, float* da, void* stream);

/* L2ContrastiveLoss (loss_functions.py:107-148): scores[a][b] = ||f1[a]-f2[b]||_2 (n x n, kept for the backward),
 * loss = (sum_{a!=b} clamp(margin - s_ab, 0)^2 [or max over b per row if max_violation] + sum_a s_aa^2) / (2n).
 * argmax_ws: n ints of scratch (max_violation only).                                                          */
int viai_l2c_fwd(const float* f1, const float* f2, int n, int d, float margin, int max_violation,
                 float* scores, float* loss, void* stream);
int viai_l2c_bwd(const float* f1, const float* f2, const float* scores, int n, int d, float margin,
                 int max_violation, const float* gscale, int* argmax_ws, float* df1, float* df2, void* stream);

/* ------------------------------------------------------------------- WaveNet
 * (wavenet_vocoder/{wavenet,modules,mixture}.py).  The dilated causal and 1x1 Conv1d layers are
 * viai_conv2d_* with kh = 1 on (B, 1, T, C) tensors; the entry points below are the remaining pieces.  */
/* torch weight_norm(dim=0): w[r][:] = g[r] * v[r][:] / ||v[r]||  (modules.py:39,59); norm: [rows] kept for bwd */
int viai_weight_norm_fwd(const float* v, const float* g, float* w, float* norm, int rows, int L, void* stream);
int viai_weight_norm_bwd(const float* dw, const float* v, const float* g, const float* norm, float* dv, float* dg,
                         int rows, int L, int accumulate, void* stream);
/* gated activation tanh(a + ca) * sigmoid(b + cb), y/yc rows = [a | b] of 2*H channels (modules.py:183-201);
 * the backward writes ONE tensor that is the gradient of both y and yc                                 */
int viai_glu_fwd(const float* y, const float* yc, float* z, long rows, int H, void* stream);
int viai_glu_bwd(const float* dz, const float* y, const float* yc, float* dy, long rows, int H, void* stream);
/* out = (a + b) * s (b may be NULL): residual / skip scaling by sqrt(0.5) (modules.py:209, wavenet.py:222-226) */
int viai_add_scale(const float* a, const float* b, float* out, float s, long n, void* stream);
int viai_relu_fwd(const float* a, float* out, long n, void* stream);
/* Dropout of the residual layers (modules.py:173-175) with a counter-based mask (csrc/dropout.hip; added under ABI 20, a purely additive
 * symbol): y[i] = keep(i) ? x[i] * scale : +0.0f, scale = (float)(1 / (1 - p)) computed in double and rounded once; a dropped element is a
 * select, +0 whatever x[i] holds.  keep(i) is a function of (seed, offset, i) alone: Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57, key
 * increments 0x9E3779B9 / 0xBB67AE85) with counter (j lo, j hi, offset lo, offset hi), key (seed lo, seed hi) gives the four words of elements
 * 4 j .. 4 j + 3; element 4 j + k is kept iff word k >= (uint32_t) floor(p * 2^32).  The backward pass is the same call on dy with the same
 * (p, seed, offset): no mask is stored.  x and y may be the same pointer; both 16-byte aligned when n >= 4.  Returns 1 (invalid value) on the
 * host, before any launch, for p < 0, p >= 1, NaN p, n < 0 or a misaligned pointer; n == 0 returns 0 without a launch.                  */
int viai_dropout(const float* x, float* y, long n, double p, unsigned long long seed, unsigned long long offset, void* stream);
/* first_conv for scalar input, Conv1d1x1(1, C): y[p][c] = x[p]*w[c] + b[c] (wavenet.py:118) and its weight grads */
int viai_outer_fwd(const float* x, const float* w, const float* b, float* y, long rows, int C, void* stream);
int viai_outer_bwd_blocks(long rows);
int viai_outer_bwd(const float* dy, const float* x, float* part, float* dw, float* db, long rows, int C, int accumulate, void* stream);
/* conditioning up-sampler: ConvTranspose2d(1,1,(KH,S),stride (1,S),padding ((KH-1)/2,0)) + ReLU on (B,F,T)
 * (wavenet.py:153-164); part: (KH*16+1)*viai_upsample_bwd_blocks() floats                               */
int viai_upsample_fwd(const float* x, const float* w, const float* bias, float* y, int B, int F, int T, int KH, int S, void* stream);
int viai_upsample_bwd_blocks(void);
int viai_upsample_bwd(const float* dy, const float* y, const float* x, const float* w, float* part, float* dx, float* dw, float* db,
                      int B, int F, int T, int KH, int S, int accumulate, void* stream);
/* DiscretizedMixturelogisticLoss (mixture.py:25-105 + loss_functions.py:43-62): yhat rows of `pitch` floats
 * ([logit|mean|log_scale] x nr_mix first), target y[row], optional mask[row];  loss = sum(l*mask)/sum(mask);
 * dyhat (optional) = d loss / d yhat.  loss_rows, wrow: [rows] scratch.                                   */
int viai_mol_loss(const float* yhat, const float* y, const float* mask, float* loss_rows, float* wrow, float* loss,
                  float* dyhat, long rows, int pitch, int nr_mix, float num_classes, float log_scale_min, void* stream);
int viai_scale_by_scalar(float* d, const float* gscale, long n, void* stream);
/* sample_from_discretized_mix_logistic (mixture.py:117-153) with injected uniforms u1[rows][nr_mix], u2[rows] */
int viai_mol_sample(const float* yhat, const float* u1, const float* u2, float* out, long rows, int pitch, int nr_mix,
                    float log_scale_min, void* stream);

/* Incremental synthesis, ONE time step (wavenet.py:322-357 loop body; conv.py:17-46 linearised convolutions).
 * Weights are plain (weight norm already applied) and linearised: w_conv[g][j*C + ci] = w[g][ci][j].
 * `step` is a device int (time index, advanced by the call); ring buffers are (B, ring_len, C) zero-initialised,
 * ring_len > 2*dilation.  All arguments are static across steps, so the call can be captured in a hipGraph.
 * B in {1,2,4,8}.  cond: (B, T, cin) up-sampled conditioning; u1 (B,T,out_ch/3), u2 (B,T): uniforms for the
 * sampler; test_inputs (B, n_test) teacher-forced prefix; out (B, T).                                       */
typedef struct viai_wn_layer {
    const float *w_conv, *b_conv, *w_c, *b_c, *w_out, *b_out, *w_skip, *b_skip;
    float* ring;
    int dilation, ring_len;
    const float* g_add;     /* optional [B][G]: the time-invariant gate contribution of global conditioning,
                               conv1x1g(embed_speakers(g)) + bias (modules.py:195-199); NULL without it (ABI v3) */
    /* fused stages (ABI v7, viai_wn_synth.fused): extended gate rows [G][K] = [Wc^0 | Wc^1 | Wc^2] for layer 0 (K = 3 C) and
     * [Wc^0 | Wc^1 | r Wc^2 | r Wc^2 Wo_prev] for layer l > 0 (K = 3 C + G/2, r = sqrt(.5), Wo_prev = the previous layer's w_out), and
     * the folded bias [G] = b_conv + b_c (+ r Wc^2 bo_prev): gate_l then needs only z_{l-1} and x_{l-1}(t), i.e. ONE dependent launch
     * per layer instead of two                                                                                                      */
    const float *w_stage, *b_stage;
} viai_wn_layer;
typedef struct viai_wn_synth {
    int B, C, G, S, cin, n_layers, out_ch, T, n_test;
    float log_scale_min;
    const viai_wn_layer* layers;            /* HOST array of n_layers descriptors (device pointers inside) */
    const float *w_first, *b_first, *w_l1, *b_l1, *w_l2, *b_l2;
    const float *cond, *test_inputs, *u1, *u2;
    float *out, *z, *skips, *yhat_dbg;      /* z: (B, G/2), skips: (B, S) scratch; yhat_dbg optional (B,T,out_ch) */
    int* step;                              /* device int, 0 before the first call: counts the calls (the step advances it itself) */
    float* z2;                              /* fused stages: second (B, G/2) buffer (z is double-buffered) */
    int fused;                              /* 1: run the fused-stage form (needs layers[].w_stage / b_stage, z2; S, out_ch, G/2 <= 256) */
    /* ---- categorical network (ABI v19): WaveNet(scalar_input=False), one-hot mu-law input and a softmax over K = out_ch classes.  All
     * zero = the mixture-of-logistics network above, so a caller that does not know these fields is unaffected.  The 24 layer stages are
     * the same; the two ends of the time step differ (wavenet.py:116-119 first conv over K input channels, :350-356 softmax / draw):
     *   w_first    [C][K]  first-conv weight, dense input form: x0[b] = w_first . row_b + b_first (a row of K floats per stream)
     *   w_first_t  [K][C]  the same weight transposed, class input form: x0[b] = w_first_t[class_b] + b_first (one contiguous row)
     * Input of time step t (the rule of wavenet.py:322-327): t < n_test: teacher-forced, class form from test_classes (B, n_test) when
     * that is given, else dense form from test_inputs (B, n_test, K); otherwise the previous step's output, class form from classes
     * when cat_quantize, else dense form from yhat_dbg; t == 0 without test inputs: init_rows (B, K) when given, else class init_class
     * (wavenet.py:308-312: 127).
     * Output of time step t: cat_softmax 1 / cat_quantize 1: a class per stream into classes (B, T) -- the inclusive prefix sum of the K
     * probabilities in class order (fp64, wave scan + carry over the four waves: fixed order), divided by its last element; the class is
     * the number of entries <= u2[b][t], at most K - 1, which is np.random.choice(K, p) from one random_sample() (wavenet.py:353-354) -- and
     * its one-hot row into yhat_dbg if given (:355-356); 1 / 0: the probabilities into yhat_dbg (:351); 0 / 0: the logits.  0 / 1 is
     * refused (the reference hands logits to np.random.choice, which raises).
     * In this mode u1 is unused, u2 (B, T) holds one uniform in [0, 1) per stream and step, yhat_dbg is (B, T, K) and REQUIRED unless
     * cat_quantize, and `out` is scratch of B (S + K) floats (the head's hidden layer, the logits).  K <= 256, K % 4 == 0, B in {1,2,4,8};
     * chain forms only: viai_wn_pipe_ok is 0 for such a descriptor.                                                                  */
    int categorical, cat_softmax, cat_quantize, init_class;
    const float* w_first_t;
    const int* test_classes;
    const float* init_rows;
    int* classes;
} viai_wn_synth;
int viai_wavenet_synth_step(const viai_wn_synth* s, void* stream);
/* host-only (no device needed): 1 if s is a categorical descriptor the chain forms run (the shape conditions above; pointers are checked
 * by the step itself) */
int viai_wn_categorical_ok(const viai_wn_synth* s);
/* mu-law classes -> waveform in [-1, 1]: y = 2 k / mu - 1, x = sign(y) ((1 + mu)^|y| - 1) / mu (the inverse of the mulaw_quantize the reference's
 * data preparation applies, utils/librivox.py:66-68; decoded there by utils/model_util.py:63-64); classes, out: n elements */
int viai_mulaw_decode(const int* classes, float* out, long n, int mu, void* stream);
/* waveform in [-1, 1] -> mu-law classes, the inverse of viai_mulaw_decode (ABI v20): y = sign(x) log1p(mu |x|) / log1p(mu),
 * class = trunc((y + 1) / 2 * mu) clamped to [0, mu] -- the closed form of the `P.mulaw_quantize` the reference's data preparation calls
 * (utils/librivox.py:66-74); x, classes: n elements */
int viai_mulaw_quantize(const float* x, int* classes, long n, int mu, void* stream);

/* ---- training the categorical network from class indices (ABI v20) ----
 * MaskedCrossEntropyLoss (loss_functions.py:24-40) on logits as rows: logits[B * T][pitch], pitch >= K, K % 4 == 0, pitch % 4 == 0 -- the NHWC
 * tensor of the network's last conv, no transpose.  target: B * T int32 classes.  With shift = s the logits row t of a stream is scored against
 * target t + s for t < T - s and the last s rows of every stream carry zero weight and zero gradient: the training convention
 * criterion(y_hat[:, :, :-1], y[:, 1:]) (train.py's __train_step) without a sliced copy.  mask (optional): B * (T - s) floats, mask[b][t]
 * weighs logits row t.  loss = sum(l * mask) / sum(mask), summed in a fixed order.  loss_rows: [B * T]; wrow: [2 * B * T] scratch (the
 * normalised row weights mask / sum(mask), then the mask as applied); dlogits (optional, rows of `pitch` floats) = d loss / d logits with
 * zeros in the columns K .. pitch.  The target logit is picked by comparing column numbers, never by addressing with the target: a target
 * outside [0, K) gives a NaN row loss where the row's mask is not 0 and is ignored where it is 0.                                        */
int viai_masked_ce_loss(const float* logits, const int* target, const float* mask, float* loss_rows, float* wrow, float* loss,
                        float* dlogits, int B, int T, int K, int pitch, int shift, void* stream);
/* first_conv of the categorical network on class indices (wavenet.py:118 applied to the one-hot rows of data_loader_utils.py:278-281):
 * h[p][:] = w[:, classes[p]] + b.  w: the layer's effective weight [C][K]; wt: [K][C] scratch that receives its transposed image (written
 * by this call, once per forward); classes: `rows` int32; h: [rows][C]; C % 4 == 0.  A class outside [0, K) gives a NaN row, not an access. */
int viai_class_embed_fwd(const int* classes, const float* w, const float* b, float* wt, float* h, long rows, int K, int C, void* stream);
/* its weight gradients, in the parameter's layout: dw[c][k] = sum over rows p with classes[p] == k of dh[p][c] (ascending p), db[c] = sum_k
 * dw[c][k].  No float atomics: the same bits on every run.  part: K * C * viai_class_embed_bwd_segments(rows) floats of scratch; C <= 1024. */
int viai_class_embed_bwd_segments(long rows);
int viai_class_embed_bwd(const float* dh, const int* classes, float* part, float* dw, float* db, long rows, int K, int C, void* stream);
/* The same time steps t0 .. t0 + n_steps - 1 launched from a host loop with the time index passed BY VALUE (ABI v5): no kernel starts
 * with a load of `*step` in front of its address arithmetic (a full memory round trip at these grid sizes).  `step` is not touched.
 * wavenet.py:237-364 incremental_forward's loop body, n_steps at a time.                                                         */
int viai_wavenet_synth_run(const viai_wn_synth* s, int t0, int n_steps, void* stream);
/* The same two calls with the teacher-forced steps chosen per stream and step (additive to ABI v20).  wavenet.py:322-327 forces a PREFIX, common
 * to the batch: test_inputs is used while t < n_test.  Here a mask `forced` (B, T) uint8 in device memory travels with test inputs that cover all
 * T steps (n_test == T is required: test_inputs (B, T) for the scalar network, test_classes (B, T) and / or test_inputs (B, T, K) for the one-hot
 * network), and the INPUT of step t of stream b is
 *     forced[b][t] != 0:  the given input -- test_inputs[b][t], or class test_classes[b][t] / row test_inputs[b][t]
 *     otherwise:          the previous output (out / classes / yhat_dbg at t - 1), or at t == 0 the start value (0.0 / init_rows / init_class).
 * Outputs are unchanged: step t writes the model's own sample, class or row at t whether or not its input was forced (wavenet.py:326-356).  A
 * step the mask does not force may hold anything in the test inputs.  forced == NULL is the prefix rule, i.e. viai_wavenet_synth_run / _step
 * themselves.  One-hot network: a step is in class form only if EVERY stream's input is a class; where the streams differ (one forced from dense
 * rows, one fed back as a class) the step takes the dense first conv and the class streams gather their weight row there.  The plain chain, the
 * fused chain (s->fused) and the device-side time index (_step_forced, for a captured graph) all take the mask; the pipelined form
 * (viai_wn_pipe_run) does not -- a caller with a mask uses these.                                                                              */
int viai_wavenet_synth_step_forced(const viai_wn_synth* s, const unsigned char* forced, void* stream);
int viai_wavenet_synth_run_forced(const viai_wn_synth* s, const unsigned char* forced, int t0, int n_steps, void* stream);

/* ---- inpainting a gap in a waveform (csrc/wn_inpaint.hip; additive to ABI v20) ----
 * Only the receptive field R in front of a gap and the gap itself need the sample-by-sample loop: the R known samples, teacher-forced, bring
 * every dilated conv's ring buffer (conv.py:17-46) to the state it has after the whole clip, and the gap runs free (wavenet.py:322-327).
 * viai_wn_window_gather cuts one window per stream out of a clip: window position t of stream b is clip time w[b] + t (w[b] = gap start - R, may
 * be negative), t < L = R + the longest gap.
 *   inputs   wav (B, n) floats and / or classes (B, n) int32 (either may be NULL, not both) -> x_out (B, L) / cls_out (B, L)
 *   cond     (B, n, cin) up-sampled conditioning (wavenet.py:291-299), or NULL -> cond_out (B, L, cin); cin % 4 == 0, 16-byte rows
 *   forced   (B, L) uint8: forced[b][t] = !(R <= t < R + len[b]) -- the steps behind a short gap are forced again (their outputs are not used)
 * Times before 0 or at and beyond n read as silence, the start-up state of wavenet.py:305-312: 0.0, class `silence_class` (127 at mu = 255) and a
 * zero conditioning row.  w, len: B int32 in device memory.                                                                                    */
int viai_wn_window_gather(const float* wav, const int* classes, const float* cond, const int* w, const int* len, float* x_out, int* cls_out,
                          float* cond_out, unsigned char* forced, int B, int n, int L, int R, int cin, int silence_class, void* stream);
/* out (B, n): out[b][i] = wav[b][i] outside the gap [g0[b], g0[b] + len[b]); inside, g = gen[b][R + i - g0[b]] with gen (B, L) the window's
 * generated samples.  fade > 0 blends the last `fade` samples of the gap linearly from generated to original (for callers that do have the
 * original there, as in evaluation): with j = i - (g0[b] + len[b] - fade) >= 0 and a = (j + 1) / (fade + 1),
 *     out[b][i] = g + a * (wav[b][i] - g)      in fp32, every operation rounded on its own.
 * fade == 0 is an exact copy on both sides.  g0, len: B int32 in device memory; out must not alias wav.                                         */
int viai_wn_splice(const float* wav, const float* gen, const int* g0, const int* len, float* out, int B, int n, int L, int R, int fade, void* stream);

/* ---- the join between the mel generator and the vocoder (csrc/inpaint_join.hip; additive to ABI v20) ----
 * The mel front end follows lws (utils/audio.py:90-108): frames = n / hop + 3 for n % hop == 0, frame j reads the clip's samples
 * [j hop - (fft - hop), j hop + hop).  The vocoder wants n == frames hop, so the clip moves right by lpad = fft - hop silent samples
 * (utils/librivox.py:92-102: lws_pad_lr, then the cut to N hop).  On that ALIGNED grid, a = i + lpad, frame j owns the samples
 * [j hop, (j + 1) hop) and its analysis window is [j hop, j hop + fft).  a0, a1 below are B int32 in device memory: one gap [a0[b], a1[b]) per
 * stream in aligned coordinates, a0[b] >= a1[b] meaning no gap.  Each call is one launch; none does arithmetic on a sample or mel value, so the
 * words that are copied keep their bits (NaN payloads included).  Output pointers need 4-byte alignment only.
 *
 * mask (B, frames) -- the memory of a (B, 1, 1, frames) time mask (1 = known, 0 = gap): a frame is damaged when its WINDOW meets the gap,
 *     mask[b][j] = (a0[b] < a1[b] && j hop < a1[b] && j hop + fft > a0[b]) ? 0 : 1
 * which is wider than the gap's own frames by the window's overhang (three frames on the left at 1024 / 256).  Any fft, hop >= 1.          */
int viai_gap_frame_mask(const int* a0, const int* a1, float* mask, int B, int frames, int fft, int hop, void* stream);
/* out (B, n + lpad): out[b][a] = 0 for a < lpad and for a0[b] <= a < a1[b], wav[b][a - lpad] otherwise.  wav (B, n); out must not alias wav. */
int viai_wav_align(const float* wav, const int* a0, const int* a1, float* out, int B, int n, int lpad, void* stream);
/* The vocoder's conditioning: real mel where the frame is clean, the generator's where it is damaged -- a select, not a blend:
 *     c[b][f][t] = mask[b][t] != 0 ? real[b][f][t] : fake[b][f][t]
 * real, fake (B, 1, F, T) contiguous, mask (B, T), c (B, F, T) (the layout wavenet.py:291-299 up-samples).  Any F, T >= 1.                     */
int viai_mel_compose(const float* real, const float* fake, const float* mask, float* c, int B, int F, int T, void* stream);

/* ---- inpainting quality metrics (csrc/metrics.hip; additive to ABI v20) ----
 * The sums behind SNR / SI-SDR over a gap in samples, L1 / PSNR / log-spectral distance over mel frames, and SSIM of two mel images.  Inputs are
 * fp32, every sum is fp64 and taken in a fixed order (thread, wave, block, then a second launch over the block partials in chunk order; no
 * atomics), over chunks laid on each stream's own region: results are the same bits from run to run, and a stream's row does not depend on the
 * batch it is in.  Each call is two launches and needs `ws`, viai_metrics_ws_doubles(kind, ...) doubles of device memory that it overwrites;
 * nothing is allocated and nothing syncs.  out and ws are 8-byte aligned.  Bad arguments (null pointers that are required, the shape rules
 * below) return hipErrorInvalidValue before any launch.
 * `where` selects frames against mask (B, T) -- the memory of a (B, 1, 1, T) time mask, 1 = known, 0 = damaged:
 *     0 every frame (mask may be NULL), 1 frames with mask == 0, 2 frames with mask != 0.                                                      */
#define VIAI_METRIC_WAVE 0
#define VIAI_METRIC_MEL_FRAMES 1
#define VIAI_METRIC_MEL_SSIM 2
/* doubles of workspace for one call: kind WAVE (B, n), MEL_FRAMES (B, F, T), MEL_SSIM (B, F, T, taps); arguments a kind does not use are ignored.
 * Pure host arithmetic; 0 for arguments the call itself refuses.                                                                             */
long viai_metrics_ws_doubles(int kind, int B, int n_or_F, int T, int taps);
/* ref, est (B, n); g0, glen: B int32 in DEVICE memory, the gap [g0[b], g0[b] + glen[b]) in samples, clamped to [0, n) on the device (never read
 * past); odd starts and lengths are legal.  out (B, 5) = {count, sum ref^2, sum est^2, sum (ref - est)^2, sum ref est} over the gap; glen <= 0
 * gives a row of zeros.  Chunk k of a gap is [g0 + 2048 k, g0 + 2048 (k + 1)).  Refuses B < 1, n < 1.                                        */
int viai_wave_gap_stats(const float* ref, const float* est, const int* g0, const int* glen, double* out, double* ws, int B, int n, void* stream);
/* ref, est (B, 1, F, T) contiguous, d = est - ref.  out (B, 4) = {frames counted, sum |d|, sum d^2, sum_t sqrt(mean_f (db_range d)^2)} over the
 * selected frames; db_range = -min_level_db (100): the normalised mel is affine in dB, so the last entry is the log-spectral distance in dB,
 * summed over frames, with no logarithm taken.  Refuses B, F, T < 1, where outside 0 .. 2, mask == NULL with where != 0.                     */
int viai_mel_frame_stats(const float* ref, const float* est, const float* mask, double* out, double* ws, int B, int F, int T, int where,
                         double db_range, void* stream);
/* SSIM (Wang et al. 2004) with the separable window win (x) win -- `taps` doubles in HOST memory, read before the call returns, expected to sum
 * to 1 -- and population moments: mu = E[.], var_x = E[x^2] - mu_x^2, cov = E[xy] - mu_x mu_y,
 *     ssim = ((2 mu_x mu_y + c1) (2 cov + c2)) / ((mu_x^2 + mu_y^2 + c1) (var_x + var_y + c2)).
 * "Valid" mode: the (F - taps + 1) x (T - taps + 1) positions whose window lies inside the image; position (f, t) reads rows f .. f + taps - 1,
 * frames t .. t + taps - 1 and belongs to its CENTRE frame t + taps / 2, which `where` tests.  out (B, 2) = {positions counted, sum of ssim}.
 * Refuses even taps, taps > 31, F < taps, T < taps.                                                                                           */
int viai_mel_ssim(const float* ref, const float* est, const float* mask, const double* win, double* out, double* ws, int B, int F, int T,
                  int taps, int where, double c1, double c2, void* stream);

/* ---- polyphase resampler: a clip at any sample rate (csrc/wav_resample.hip; additive to ABI v20) ----
 * sr_in -> sr_out with g = gcd, L = sr_out / g, M = sr_in / g, s = min(1, L / M), c = rolloff s, W = zeros / s, H = ceil(W), T = 2 H + 1.
 * Output k sits at input time k M / L; with i0 = floor(k M / L) and r = (k M) mod L
 *     y[k] = sum_{j = 0 .. T - 1} x[i0 - H + j] h_r[j],     h_r[j] = c sinc(c t) kaiser(t / W),     t = r / L - (j - H),
 * sinc(v) = sin(pi v) / (pi v), kaiser(u) = I0(beta sqrt(1 - u^2)) / I0(beta) for |u| < 1 and 0 otherwise, x zero outside [0, length).
 * TABLE LAYOUT: period order, tap-major.  Row q = k mod L of the table holds phase r = (q M) mod L, first[q] = floor(q M / L), and
 * tap j of row q is taps[j * L + q]: output k = p L + q reads x[p M + first[q] - H + j] against taps[j * L + q], so consecutive outputs of one
 * period read consecutive words.  L * T floats and L ints.
 * Plans whose table L * T exceeds VIAI_WAV_RESAMPLE_MAX_TABLE words are refused, by the plan and by the launch.                              */
#define VIAI_WAV_RESAMPLE_MAX_TABLE 4194304
/* pure arithmetic.  Refuses (hipErrorInvalidValue) rates below 1, zeros < 1, null pointers and a table over the cap.                          */
int viai_wav_resample_geom(int sr_in, int sr_out, int zeros, int* L, int* M, int* H, int* T);
/* the launch form viai_wav_resample takes for a plan (L, M, H); pure arithmetic, touches no device.  A tile is lt * g * pp consecutive outputs
 * and stages span = floor((lt g pp - 1) M / L) + 2 H + 3 words of LDS (at most 16 384).
 *   pp = 4  the period form, L <= 512: lt = L, work item w keeps q = w mod L and takes the periods w / L + g {0, 1, 2, 3} of the tile; g = 1 when
 *           its span fits, a larger g <= max(1, 1024 / L) only where it fills the block's passes better by more than a hundredth
 *   pp = 1  the consecutive form, L > 512 or no period tile fits: g = 1, lt = the largest of 1024, 512, 256, 128, 64 whose span fits
 *   pp = 0  no tile fits (lt = g = span = 0): viai_wav_resample refuses the plan
 * Returns 0 in all three cases; refuses (hipErrorInvalidValue) null pointers, L or M < 1, H < 0.                                              */
int viai_wav_resample_form(int L, int M, int H, int* pp, int* lt, int* g, int* span);
/* the table in HOST memory: taps L * T floats, first L ints, computed in fp64 (I0 by its power series) and rounded once to fp32.  Refuses what
 * the plan refuses, rolloff outside (0, 1] and beta outside [0, 700).                                                                         */
int viai_wav_resample_taps(int sr_in, int sr_out, int zeros, double rolloff, double beta, float* taps, int* first);
/* ceil(n L / M), the outputs of n input samples; 0 for n < 0 or L, M < 1                                                                      */
long viai_wav_resample_out_len(long n, int L, int M);
/* the resampler's counterpart of gap_frames: the outputs k in [0, m) whose filter support [i0 - H, i0 + H] meets the input gap [g0, g1):
 * k0 = max(0, ceil((g0 - H) L / M)), k1 = min(m, ceil((g1 + H) L / M)); an empty gap (g1 <= g0), or one no output meets, gives (0, 0).
 * Pure host arithmetic in 64 bits.                                                                                                            */
int viai_gap_at_rate(long g0, long g1, int L, int M, int H, long m, long* k0, long* k1);
/* x (B, x_stride) fp32; lengths (B,) int32 in DEVICE memory or NULL (every row x_stride long), clamped to [0, x_stride]: samples at and beyond a
 * row's length read as zero.  taps, first: the table above in DEVICE memory.  y (B, y_stride) fp32.  o0, o1 (B,) int32 in DEVICE memory or NULL:
 * the call writes the outputs k in [o0[b], o1[b]) intersected with [0, m) (NULL: [0, m)) and leaves every other element of y untouched.
 * One launch for the batch, nothing allocated, nothing syncs.  Each output is the fp32 chain acc = fma(x, h, acc), j = 0 .. T - 1, from +0:
 * y[b][k] has the same bits for a row alone, in any batch and under any window.  Outputs past ceil(length L / M) follow the same formula: they
 * decay over the filter's support and are exact zeros from ceil((length + H) L / M) on.
 * Refuses before any launch: x, taps, first or y NULL; B, m, L, M or T < 1; T != 2 H + 1; x_stride < 1; y_stride < m; a table over the cap;
 * a plan whose smallest tile (64 outputs and 2 H + 3 samples of halo) does not fit 64 KiB of LDS.                                            */
int viai_wav_resample(const float* x, const int* lengths, const float* taps, const int* first, float* y, const int* o0, const int* o1, int B,
                      long x_stride, long y_stride, int m, int L, int M, int H, int T, void* stream);

/* ---- gap detection: where a waveform is damaged (csrc/gap_detect.hip; additive to ABI v20) ----
 * A sample is DAMAGED when it is not finite, or |x| <= threshold, or (clip > 0 and |x| >= clip).  threshold = 0 means exact zeros, -0.0 included;
 * clip = 0 switches the clipping test off.  For row b, len = clamp(lengths[b], 0, n), or n when lengths is NULL:
 *   1  a RAW RUN is a maximal interval [s, e) of damaged samples inside [0, len); samples at and beyond len do not exist, they neither start nor
 *      extend a run;
 *   2  a raw run is KEPT when e - s >= min_len;
 *   3  kept runs are taken in order of position, and a kept run JOINS the one before it when s - e_prev <= merge_within; the joined run is
 *      [s_first, e_last).  The distance is between kept runs: a dropped short run between them counts as ordinary samples.  With
 *      merge_within = 0 nothing joins (two maximal runs are at least one sample apart);
 *   4  count[b] is the number of runs after 3 and may exceed K; start[b][k], length[b][k] hold the first K of them in position order, and the
 *      entries k >= min(count[b], K) are written as 0.
 * count (B,), start and length (B, K) are int32.  The results are exact, the same from run to run, and the same for a row alone or in any batch:
 * the order comes from an exclusive sum over the tiles of a row, no atomic is involved.
 * One block owns VIAI_GAP_DETECT_TILE samples of one row (tile t of a row is [t TILE, (t + 1) TILE), counted from the row's first sample).      */
#define VIAI_GAP_DETECT_TILE 4096
/* bytes of workspace for one call: the 1-bit-per-sample mask and a small table per tile.  Pure host arithmetic; 0 for arguments the call itself
 * refuses (B, n or K < 1, n >= 2^31, more than 2^31 - 1 tiles in the batch).                                                                   */
long viai_gap_detect_ws_bytes(int B, long n, int K);
/* wav (B, stride) fp32, row b at wav + b stride, in DEVICE memory; lengths (B,) int32 in DEVICE memory or NULL; count, start, length in DEVICE
 * memory; ws: viai_gap_detect_ws_bytes(B, n, K) bytes of device memory, 8-byte aligned, overwritten.  THREE launches for the whole batch (mask and
 * per-tile summary; one block per row over the summaries; the runs written in place); nothing is allocated and nothing syncs.  Rows are read with
 * 16-byte loads where wav + b stride is 16-byte aligned and with 4-byte loads otherwise; no sample at or beyond len is read.
 * Refuses with hipErrorInvalidValue before any launch: wav, count, start, length or ws NULL; B, n or K < 1; n >= 2^31; stride < n; min_len < 1;
 * merge_within < 0; a negative or NaN threshold; a negative or NaN clip; wav not 4-byte or ws not 8-byte aligned; more than 2^31 - 1 tiles.   */
int viai_gap_detect(const float* wav, const int* lengths, long stride, int B, long n, float threshold, float clip, int min_len, int merge_within,
                    int K, int* count, int* start, int* length, void* ws, void* stream);
/* the same rule stated sample by sample in plain C++, every pointer in HOST memory: the statement the kernels are tested against, and the call for
 * a user without a GPU.  Same refusals (ws and the alignment rules apart).                                                                    */
int viai_gap_detect_host(const float* wav, const int* lengths, long stride, int B, long n, float threshold, float clip, int min_len,
                         int merge_within, int K, int* count, int* start, int* length);

/* ---- short gaps: Burg autoregressive interpolation (csrc/ar_fill.hip, csrc/viai_ar_rule.h; additive to ABI v20) ----
 * Every listed gap of every row is filled from the clean samples on its two sides: an all-pole model is fitted to each side (Burg's method),
 * extrapolated into the gap -- forward from the left, backward from the right -- and the two predictions are cross-faded.  fp64 arithmetic of
 * + - * / only, each operation rounded once, every sum in a stated order: the kernel and the host mirror call the same functions of
 * csrc/viai_ar_rule.h and give the same bits.
 * For row b, len = clamp(lengths[b], 0, n) (n when lengths is NULL) and listed = min(max(count[b], 0), K).  Gap k < listed is
 * [s, e) = [start[b][k], start[b][k] + length[b][k]), L = e - s:
 *   SKIPPED   (filled = 0, no sample written) when L < 1, L > max_len, s < 0 or e > len; filled[b][k] = 0 for k >= listed as well.
 *   CONTEXT   left [max(s - context, start[b][k-1] + length[b][k-1] if k > 0, 0), s), right [e, min(e + context, start[b][k+1] if k + 1 < listed,
 *             len)); an empty interval where the bounds cross.  The neighbours count whether they are skipped or not, so with lists in position
 *             order a context never holds a sample of a listed gap: what a block reads is disjoint from what every block writes, and out may
 *             be wav itself.  A non-finite context sample reads as 0.0.
 *   ORDER     a side with C context samples has p = min(order, C / 2) (integer division) and is usable iff p >= 1.
 *   FIT       Burg on x[0 .. C), the right side on its context time-reversed (x[j] = row[e + C - 1 - j]): f = x[1:], b = x[:-1], a = [1]; per
 *             stage k = -2 <f, b> / (<f, f> + <b, b>), 0 when the denominator is 0; a <- [a, 0] + k reverse([a, 0]); f' = (f + k b)[1:],
 *             b' = (b + k f)[:-1]; p stages.  No clamp, no window.
 *   SUMS      each of the three dot products of a stage: 256 partials, partial t the terms i = t, t + 256, ... in ascending i from +0.0, each
 *             term one rounded product added with one rounded sum; then the adjacent pairwise tree: for o = 1, 2, 4, ..., 128,
 *             part[t] += part[t + o] for every t that is a multiple of 2 o.
 *   EXTRAPOLATE  x^[i] = 0.0 - sum_{j = 1 .. p} a_j x^[i - j], i = 0 .. L - 1, seeded with the last p context samples.  The sum: 64 partials,
 *             partial l = a_{l+1} x^[i-l-1] (+ a_{l+65} x^[i-l-65]) over the terms with j <= p, +0.0 without one, then the same tree over 64.
 *             fwd[i] is step i from the left; bwd[i] is step L - 1 - i of the reversed right side.
 *   BLEND     u = (i + 0.5) / L, w = 1 - (u u) (3 - 2 u), out = w fwd + (1 - w) bwd, rounded to fp32 once.  Left side only: out = fwd; right
 *             only: out = bwd; neither: out = 0.0.
 *   filled    1 both sides, 2 left only, 3 right only, 4 no context (zeros written), 0 skipped or not listed.
 * wav (B, stride) fp32, lengths (B,), count (B,), start / length (B, K) int32 and filled (B, K) int32 in DEVICE memory, as viai_gap_detect leaves
 * them; out (B, out_stride) fp32: ONLY the samples of filled gaps are written, so the caller copies wav to out first or passes out = wav.  ONE
 * launch, one block of 256 threads per (row, gap index), no atomics, no workspace, nothing synced; dynamic LDS
 * 8 (max(4 context, 2 (128 + max_len)) + 540) bytes per block, 135 392 at the limits.
 * Refuses with hipErrorInvalidValue before any launch: a NULL pointer (lengths excepted); B or K < 1; B K > 2^31 - 1; n < 1 or n >= 2^31;
 * stride or out_stride < n; order outside 1 .. 128; context outside 2 .. 4096; max_len outside 1 .. 4096; wav or out not 4-byte aligned.       */
int viai_ar_fill(const float* wav, const int* lengths, long stride, int B, long n, const int* count, const int* start, const int* length, int K,
                 int order, int context, int max_len, float* out, long out_stride, int* filled, void* stream);
/* the same rule with plain loops from the same header, every pointer in HOST memory.  Same refusals (the alignment rule apart).                */
int viai_ar_fill_host(const float* wav, const int* lengths, long stride, int B, long n, const int* count, const int* start, const int* length,
                      int K, int order, int context, int max_len, float* out, long out_stride, int* filled);
/* the fit alone, for pinning: x (C,) fp32 in HOST memory, 0 <= C <= 4096 -> a[0 .. order] fp64 (a[0] = 1, zeros behind a[p]) and
 * *p = min(order, C / 2).  Refuses a NULL pointer, C outside 0 .. 4096, order outside 1 .. 128.                                                */
int viai_ar_fit_host(const float* x, int C, int order, double* a, int* p);

/* ---- crackle and short gaps: Janssen's least-squares AR interpolation (csrc/janssen_fill.hip, csrc/viai_janssen_rule.h on csrc/viai_ar_rule.h;
 * additive to ABI v20) ----
 * viai_ar_fill treats every listed run on its own and cuts its contexts at the neighbouring runs; where runs are dense (crackle) the contexts
 * shrink to a few samples.  Here runs that lie within `context` of each other form a CLUSTER, one all-pole model is fitted to the cluster's whole
 * window with the current estimates in place, ALL its missing samples are solved for jointly (Janssen, Veldhuis and Vries 1986), and that is
 * repeated `iters` times.  fp64 arithmetic of + - * / and comparisons only, each operation rounded once, every sum in a stated order: the
 * kernel and the host mirror call the same functions of csrc/viai_janssen_rule.h and give the same bits.
 * For row b, len = clamp(lengths[b], 0, n) (n when lengths is NULL) and listed = min(max(count[b], 0), K).  Entry k < listed is
 * [s, e) = [start[b][k], start[b][k] + length[b][k]), L = e - s; front_k = max(0, start[b][j] + max(length[b][j], 0) over j < k) is the end of
 * everything listed in front of it (for lists in position order: the end of entry k - 1).
 *   USABLE    1 <= L <= max_len, s >= front_k and e <= len.  Every other entry, and every k >= listed, is SKIPPED: filled = 0, no sample written.
 *             A skipped entry still is a wall for its neighbours' windows.
 *   CLUSTERS  integers only.  A cluster opens at the first usable entry not yet in one.  The next entry j joins iff it is usable,
 *             s_j - e_last < context, M + L_j <= 1024, (M + L_j) (order + 1) <= 8192 and (e_j - s_first) + 2 context <= 4096 (M: the unknowns so
 *             far).  An entry that does not join closes the cluster; if usable it opens the next one.
 *   WINDOW    [max(s_first - context, front_first, 0), max(min(e_last + context, start of the entry behind the last member if listed, len),
 *             e_last)); W its size, M its unknowns at window positions t_0 < ... < t_{M-1}.  No window holds an unknown of another cluster, so
 *             out may be wav itself.  A non-finite known sample reads as 0.0; samples outside the window count as 0.0.
 *   ITERATE   the unknowns start at 0.0 and stay fp64 between iterations.  p = min(order, W / 2); p < 1: zeros are written, filled = 4.
 *             iters times: a[0 .. p] = Burg's fit of viai_ar_fill (FIT and SUMS above, unchanged) on the window with the current estimates;
 *             b_l = sum_{k = 0 .. p - l} a_k a_{k+l}; G_ij = b_{|t_i - t_j|} when |t_i - t_j| <= p, else 0; r_i = 0.0 - sum_{l = -p .. p}
 *             b_{|l|} x0[t_i + l] over the positions inside the window, x0 the window with 0.0 at the unknowns; G = L D L^T, solve, the
 *             unknowns <- the solution.  A pivot d_j that is not > 0.0 or not finite stops everything: the estimates of the last completed
 *             iteration stay (zeros when none completed), filled = 5.
 *   SUMS      b_l: ascending k from +0.0, acc = acc + a_k a_{k+l} (one rounded product, one rounded sum).  r_i: ascending l from +0.0 in the same
 *             way (an unknown's term adds its 0.0), then 0.0 - acc.
 *   SOLVE     inside the index band of p sub-diagonals (|t_i - t_j| >= |i - j|: G and all fill lie there), right-looking: for j = 0 .. M - 1:
 *             d_j = A_jj; for i = j + 1 .. min(j + p, M - 1): c_i = A_ij, l_i = c_i / d_j, z_i = z_i - l_i z_j (z starts as r); then
 *             A_ik = A_ik - l_i c_k for j < k <= i (the product is l_i c_k, not l_i d_j l_k).  So every element takes its updates one at a
 *             time in ascending j.  Then y_i = z_i / d_i, and for j = M - 1 .. 1: x_i = x_i - l_ji x_j for i = j - 1 .. max(j - p, 0).
 *   WRITE     out[t_i] = (float)x_i, one rounding, at the unknowns only.
 *   filled    the same for every member of a cluster: 1 solved for all iters, 4 no model, 5 stopped at a pivot; 0 skipped or not listed.
 * Memory as viai_ar_fill.  ONE launch, one block of 256 threads per (row, entry index): the block of a cluster's first member does the cluster
 * and writes filled of all members, a skipped entry's block writes its 0, every other block returns at once; no atomics, no workspace, nothing
 * synced; dynamic LDS 123 056 bytes per block whatever the arguments (the lists are read on the device, so the host cannot know W or M).
 * Refuses with hipErrorInvalidValue before any launch: what viai_ar_fill refuses, with context outside 2 .. 1024, iters outside 1 .. 16 and
 * max_len outside 1 .. min(1024, 8192 / (order + 1), 4096 - 2 context).                                                                      */
int viai_janssen_fill(const float* wav, const int* lengths, long stride, int B, long n, const int* count, const int* start, const int* length,
                      int K, int order, int context, int max_len, int iters, float* out, long out_stride, int* filled, void* stream);
/* the same rule with plain loops from the same header, every pointer in HOST memory.  Same refusals (the alignment rule apart).                */
int viai_janssen_fill_host(const float* wav, const int* lengths, long stride, int B, long n, const int* count, const int* start,
                           const int* length, int K, int order, int context, int max_len, int iters, float* out, long out_stride, int* filled);
/* USABLE, CLUSTERS and WINDOW alone, for pinning; HOST memory.  Per entry (B, K) int32: leader = the index of its cluster's first member (-1:
 * skipped, the other three are then 0), the window [win_lo, win_hi) and the cluster's M.                                                       */
int viai_janssen_plan_host(const int* lengths, int B, long n, const int* count, const int* start, const int* length, int K, int order,
                           int context, int max_len, int* leader, int* win_lo, int* win_hi, int* unknowns);

/* ---- declipping: bound-constrained Janssen AR restoration (csrc/declip.hip, csrc/viai_declip_rule.h on csrc/viai_janssen_rule.h and
 * csrc/viai_ar_rule.h; additive to ABI v20) ----
 * A clipped sample carries two facts a dropout does not: its sign, and a lower bound on its magnitude.  viai_janssen_fill uses neither, and
 * clipped voiced sound (a run at every peak) makes its clusters close on capacity, each a wall for the next.  Here the same joint solve runs
 * under the bounds, on windows that are NOT cut at neighbouring entries, and several launches (SWEEPS) hand the estimates of one cluster to the
 * windows of the others.  fp64 arithmetic of + - * / and comparisons only, each operation rounded once, every sum one of viai_janssen_fill's:
 * the kernel and the host mirror call the same functions of csrc/viai_declip_rule.h and give the same bits.
 * Three buffers: ref (B, stride) is the clip as recorded and gives the bounds; src (B, stride) holds the current estimates and is read
 * everywhere (the first sweep passes src = ref); out (B, out_stride) is written at the unknowns only and must not overlap src or ref.  Rows,
 * len, listed, entries and front_k as for viai_janssen_fill.
 *   USABLE, CLUSTERS  exactly those of viai_janssen_fill, limits and capacity tests included.
 *   WINDOW    [max(s_first - context, 0), min(e_last + context, len)); W <= 4096 by the cluster rule.  It is NOT cut at neighbouring entries:
 *             samples of other clusters' entries (and of skipped entries) inside it are knowns, read from src -- the recorded values in the
 *             first sweep, the previous sweep's estimates later.  That is why out may not be src.  A non-finite known reads as 0.0.
 *   BOUND     for unknown i at window position t_i, c_i = ref[t_i] in fp64, a non-finite one read as 0.0.  c_i > 0: x_i >= c_i; c_i < 0:
 *             x_i <= c_i; c_i == 0 (a dropout, a non-finite sample): free.  x VIOLATES when the comparison is not true (so a NaN violates).
 *   START     the estimates start at src[t_i] (fp64, non-finite as 0.0), not at 0.0.  p = min(order, W / 2); p < 1: the start values are
 *             written, filled = 4.
 *   ITERATE   iters times:
 *             fit     a[0 .. p] = Burg's fit of viai_ar_fill on the window with the current estimates; b_l as viai_janssen_fill.  All pins
 *                     are cleared.
 *             solve   viai_janssen_fill's solve for all M unknowns (G, r, L D L^T, unchanged; x0 holds 0.0 at the unknowns).
 *             pin     up to `rounds` times: every unknown that is not pinned and violates becomes PINNED: x_i = c_i, and x0[t_i] = c_i.  If
 *                     none was pinned in this round, or no unknown is left free, the rounds end.  Otherwise the free unknowns, compacted in
 *                     position order f(0) < f(1) < ... < f(M' - 1), are solved again with the same a: G'_qr = b_{|t_f(q) - t_f(r)|} inside p,
 *                     r'_q = 0.0 - sum_l b_{|l|} x0[t_f(q) + l] (the pinned ones are knowns of value c), the same banded L D L^T over M'.
 *             clamp   if rounds >= 1: every unknown that still violates is set to c_i.  Then the estimates <- x, and x0 is 0.0 at every
 *                     unknown again.  With rounds = 0 nothing is pinned and nothing is clamped: the unconstrained wide-window solve.
 *             A pivot that is not > 0.0 or not finite, in ANY solve, stops the cluster: the estimates of the last completed iteration stay
 *             (the start values when none completed), filled = 5.
 *   SUMS      those of viai_janssen_fill.  The compaction is an exclusive count in position order: integers only.
 *   WRITE     out[t_i] = (float)x_i, one rounding, at the unknowns only.  Rounding is monotone and c_i is an fp32 value, so with rounds >= 1
 *             every sample written with filled = 1 satisfies its bound in fp32.
 *   filled    as viai_janssen_fill: 1, 4, 5, and 0 for skipped or not listed.
 * This is an active-set HEURISTIC WITHOUT RELEASE, not an exact quadratic program: a pinned unknown stays pinned until the next fit even when
 * the re-solve would let it go, and the clamp is a projection.
 * ONE launch per call (a sweep), one block of 256 threads per (row, entry index) as viai_janssen_fill; no atomics (the pin bitmap is a word per
 * wave, the compaction ballots and a four-wave exclusive sum), no workspace, nothing synced; dynamic LDS 143 696 bytes per block.
 * Refuses with hipErrorInvalidValue before any launch: what viai_janssen_fill refuses (for ref, src and out alike), rounds outside 0 .. 8,
 * and out overlapping src or ref ([p, p + 4 ((B - 1) stride + n)) as byte ranges).                                                              */
int viai_declip(const float* ref, const float* src, const int* lengths, long stride, int B, long n, const int* count, const int* start,
                const int* length, int K, int order, int context, int max_len, int iters, int rounds, float* out, long out_stride, int* filled,
                void* stream);
/* the same rule with plain loops from the same header, every pointer in HOST memory.  Same refusals (the alignment rule apart).                */
int viai_declip_host(const float* ref, const float* src, const int* lengths, long stride, int B, long n, const int* count, const int* start,
                     const int* length, int K, int order, int context, int max_len, int iters, int rounds, float* out, long out_stride,
                     int* filled);

/* ---- clicks: impulsive damage found in a prediction residual (csrc/click_detect.hip, csrc/viai_click_rule.h; additive to ABI v20) ----
 * A click is neither silent nor clipped nor non-finite, so viai_gap_detect cannot see it.  Here an all-pole model is fitted to a stretch of the
 * signal, the signal is run through the inverse (prediction-error) filter, and a click is where the squared residual stands far above its own
 * robust scale.  fp64 arithmetic of + - * / and comparisons only, each operation rounded once, every sum in a stated order (no sqrt, no median):
 * the kernels and the host mirror call the same functions of csrc/viai_click_rule.h and csrc/viai_ar_rule.h and give the same lists.
 * For row b, len = clamp(lengths[b], 0, n) (n when lengths is NULL).  The row is cut into the tiles of viai_gap_detect (VIAI_GAP_DETECT_TILE = 4096
 * samples).  For the tile [t0, t0 + C), C <= 4096, xs(i) the row's sample i in fp64 with a non-finite one read as 0.0:
 *   FIT       p = min(order, C / 2) (integer division); a[0 .. p] is Burg's fit of viai_ar_fill (FIT and SUMS above, unchanged) on the tile's own C
 *             samples xs(t0 .. t0 + C - 1).  p < 1: nothing in the tile is judged.
 *   RESIDUAL  every sample g = t0 + i of the tile with g >= p is JUDGED: e = sum_{j = 0 .. p} a[j] xs(g - j), accumulated from +0.0 in ascending j,
 *             each term one rounded product added with one rounded sum; the sum reaches back into the previous tile's samples.  q = e e.  Samples
 *             with g < p (the head of the row) are not judged.
 *   SCALE     var_0 = sum(q) / cnt over the judged samples of the tile, cnt an integer converted to double; then `passes` times (0 .. 4)
 *             var_{r+1} = sum(q | q <= kk var_r) / count(q <= kk var_r), a count of 0 leaving var as it was (and var_0 = 0.0 when cnt = 0).
 *             kk = (double)k (double)k.  Each sum: 256 partials, partial t the tile-local indices i = t, t + 256, ... in ascending i from +0.0 (the
 *             samples that do not take part are left out), then the adjacent pairwise tree of SUMS above.
 *   FLAG      a judged sample is flagged when q > kk max(var, ff), ff = (double)floor (double)floor: floor is an amplitude below which nothing
 *             is a click.  A non-finite sample is always flagged, judged or not.
 *   GUARD     the damage mask is the flags widened by `guard` samples on both sides: sample i is damaged when a flag lies in
 *             [i - guard, i + guard].  The widening crosses tiles and never leaves [0, len).  A flag is always judged by the tile that holds the
 *             sample, and the widening works on the flags alone.
 *   RUNS      the mask goes through steps 1 to 4 of viai_gap_detect's rule with "damaged" read from the mask: min_len, merge_within, K, count the
 *             true number.  count (B,), start and length (B, K) int32: the tensors of viai_gap_detect, with the same meaning, and what
 *             viai_ar_fill and viai_pcm_patch read.
 * The lists are exact integers, the same from run to run and for a row alone or in any batch.  Joining them with the lists of viai_gap_detect
 * into one is not done here.                                                                                                                  */
/* bytes of workspace for one call: the raw flags, the mask (1 bit per sample each) and viai_gap_detect's table per tile.  0 for arguments the
 * call itself refuses (B, n or K < 1, n >= 2^31, more than 2^31 - 1 tiles in the batch).                                                       */
long viai_click_detect_ws_bytes(int B, long n, int K);
/* wav (B, stride) fp32 and lengths (B,) int32 or NULL in DEVICE memory; count, start, length in DEVICE memory; ws: viai_click_detect_ws_bytes(B, n,
 * K) bytes of device memory, 8-byte aligned, overwritten.  FOUR launches for the whole batch: one block of 256 threads per tile (fit, residual,
 * scale, raw flags; 67 744 bytes of dynamic LDS, two blocks per CU), one wave per tile (widening, mask, summary), then launches 2 and 3 of
 * viai_gap_detect.  No atomics, nothing allocated, nothing syncs; rows need 4-byte alignment only; no sample at or beyond len is read.
 * Refuses with hipErrorInvalidValue before any launch: wav, count, start, length or ws NULL; B, n or K < 1; n >= 2^31; stride < n; order outside
 * 1 .. 128; k not > 0 or not finite; passes outside 0 .. 4; guard outside 0 .. 64; a negative or NaN floor; min_len < 1; merge_within < 0; wav
 * not 4-byte or ws not 8-byte aligned; more than 2^31 - 1 tiles.                                                                              */
int viai_click_detect(const float* wav, const int* lengths, long stride, int B, long n, int order, float k, int passes, int guard, float floor,
                      int min_len, int merge_within, int K, int* count, int* start, int* length, void* ws, void* stream);
/* the same rule with plain loops from the same headers, every pointer in HOST memory.  Same refusals (ws and the alignment rules apart).       */
int viai_click_detect_host(const float* wav, const int* lengths, long stride, int B, long n, int order, float k, int passes, int guard,
                           float floor, int min_len, int merge_within, int K, int* count, int* start, int* length);

/* ---- video front end: motion crop, square pad, resize (csrc/video_prep.hip; additive to ABI v20) ----
 * Raw uint8 frames and flow maps of any H x W in, the blocks the generator's visual branch consumes out: `find_cluster`, `crop_image` and
 * `padding_square` of Data_loaders/Image_preprocess.py:168-229,256-268 and the resize / flip / normalise / crop of
 * Data_loaders/audio_loader.py:185-245.  Everything is integer arithmetic up to the last divide, so every result is exact.
 *
 * MOTION BOX.  flow_x, flow_y are (N, H, W) uint8.
 *   1  S[y][x] = sum over the N frames of |fx - 127| + |fy - 127|, int32.  A pixel is in the MASK when S > 2 N (strict).
 *   2  a column x is OCCUPIED when any pixel of it is in the mask; rows alike.
 *   3  per axis, on the ascending list o[0 .. len) of occupied indices (`find_cluster`): min_idx = 0; repeat len - 1 times: if o[min_idx] + 5 is
 *      not an occupied index, min_idx += 1.  max_idx = len - 1; repeat len - 1 times: if o[max_idx] - 5 is not an occupied index, max_idx -= 1.
 *      min = o[min_idx], max = o[max_idx]; if min > max then max = min.  In closed form (what the kernel evaluates; the tests hold the two
 *      against each other): min is the first occupied v whose v + 5 is occupied, or the last occupied index when there is none; max is the
 *      last occupied v whose v - 5 is occupied, or the first occupied index when there is none.
 *   4  an empty mask gives min = max = 0 on both axes.
 *   5  box = (w_min, w_max, h_min, h_max, ok), int32, ok = (w_max - w_min >= min_extent) && (h_max - h_min >= min_extent).  The reference uses
 *      min_extent = 50 and deletes the clip when ok is 0.
 * CROP.  Rows [h_min, h_max) x columns [w_min, w_max): the upper bounds are EXCLUSIVE, as in the reference.  Before any address is formed the box
 * is clamped to the frame (w_min to [0, W], w_max to [w_min, W], rows alike).  When ok == 0, or the clamped crop is empty, the WHOLE FRAME is
 * taken instead: a choice made here for inference (the reference has no such clip left); `ok` tells a caller that wants to drop the clip.
 * SQUARE PAD (`padding_square`).  ch x cw is the crop, side = max(ch, cw), d = side - min(ch, cw): the shorter axis gets d / 2 (integer division)
 * pixels of grey 127 in front and d - d / 2 behind, on every channel.  The pad is a coordinate test, it is never stored.
 * RESIZE side x side -> R x R: OpenCV's INTER_LINEAR for 8-bit images stated as integer arithmetic; one table serves both axes.  For d in [0, R):
 *   f = float32((d + 0.5) * (side / R) - 0.5), the quotient, the product and the difference in fp64, each rounded once (no fused multiply-add);
 *   s = floor(f), a = f - s in fp32; if s < 0: s = 0, a = 0; if s >= side - 1: s = side - 1, a = 0;
 *   c0 = rint((1 - a) * 2048), c1 = rint(a * 2048), fp32, round-half-even; the second tap is s' = min(s + 1, side - 1).
 *   horizontal  h = p[s] * c0 + p[s'] * c1 in int32, with the table entry of the output column;
 *   vertical    q = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2 with (b0, b1) the entry of the output row and h0, h1 the
 *               horizontal results on source rows s and s'; q is stored as min(q, 255).
 * OpenCV is not a dependency and is not available to the tests, so parity with cv2.resize is RESTATED here, not pinned by a test.  Pinned are:
 * identity for side == R, constant images stay constant (255 included), and at most 1 grey level from fp64 bilinear (align_corners = False).
 * The reference writes the cropped frames to JPEG and reads them back before it resizes; that lossy round trip is deliberately not reproduced.
 * FINISH: exactly viai_frames_prep on the R x R image: flip left to right, rows [crop_x, +size) and columns [crop_y, +size), (q - 127) / 128.
 *
 * SOURCES.  src1 == NULL: src0 is (N, H, W, C) uint8, channels interleaved; bgr != 0 reverses the channel axis (output channel c reads source
 * channel C - 1 - c: the reference's cvtColor).  src1 != NULL: C must be 2, src0 and src1 are (N, H, W) planes that give channels 0 and 1
 * (flow_x, flow_y); bgr swaps them.  frame_stride is the distance between frames in bytes, >= H W C (H W for planes and for the motion box).
 * frames_index: n int32 in DEVICE memory, the frames to resample in output order (repeats allowed), or NULL for frames 0 .. n - 1 (n <= N);
 * an index outside [0, N) is clamped, never followed.                                                                                         */
#define VIAI_MOTION_TILE_W 256 /* pixels of a row one wave owns in the motion pass: 16 lanes x 16 pixels */
#define VIAI_MOTION_TILE_H 4   /* rows of a tile: 4 x 16 lanes = one wave                                 */
/* bytes of workspace of viai_motion_box: one occupancy byte per column per tile row and per row per tile column.  0 for refused H, W.       */
long viai_motion_box_ws_bytes(int H, int W);
/* Two launches, no atomics, nothing allocated, nothing synced, no copy to the host.  1: one wave per 4 x 256 tile streams both stacks once
 * (16-byte loads where a row's 16 pixels are 16-byte aligned and inside the row, byte loads otherwise), keeps the 16 int32 sums of a lane in
 * registers over the frames and writes the tile's row and column flags with plain stores.  2: one block ORs the flags, applies rule 3 to both
 * axes and writes box (5 int32, DEVICE memory).  ws: viai_motion_box_ws_bytes(H, W) bytes of device memory, overwritten.
 * Refuses with hipErrorInvalidValue before any launch: a NULL pointer; N < 1 or N > 2^22; H or W < 1 or >= 2^15; frame_stride < H W;
 * min_extent < 0.                                                                                                                             */
int viai_motion_box(const unsigned char* flow_x, const unsigned char* flow_y, long frame_stride, int N, int H, int W, int min_extent, int* box,
                    void* ws, void* stream);
/* the two launches of viai_motion_box on their own (viai_motion_box is one after the other): the flags of every tile into ws, and the box from
 * the flags in ws.  For a caller that times or reuses them; same refusals.                                                                    */
int viai_motion_flags(const unsigned char* flow_x, const unsigned char* flow_y, long frame_stride, int N, int H, int W, void* ws, void* stream);
int viai_motion_box_of_flags(const void* ws, int H, int W, int min_extent, int* box, void* stream);
/* rules 1 - 5 pixel by pixel and rule 3 as the sequential walk, in plain C++, every pointer in HOST memory.  Same refusals.                 */
int viai_motion_box_host(const unsigned char* flow_x, const unsigned char* flow_y, long frame_stride, int N, int H, int W, int min_extent,
                         int* box);
/* bytes of workspace of viai_video_resize_u8 / viai_video_prepare: the resolved crop and the R-entry coefficient table.  0 for a refused R.   */
long viai_video_prep_ws_bytes(int R);
/* crop + pad + resize of n frames -> out uint8 (n, R, R, C), DEVICE memory.  box: 5 int32 in DEVICE memory (viai_motion_box's, or the caller's).
 * Two launches: one block resolves the crop from box and makes the table once (fp64 / fp32 as in the rule) in ws; the second resamples.
 * Refuses before any launch: a NULL src0, box, out or ws; C outside 1..4; src1 with C != 2; N < 1 or > 2^22; n < 1; n > N without frames_index;
 * H or W < 1 or >= 2^15; R < 1 or > 2^13; a frame_stride below one frame.                                                                    */
int viai_video_resize_u8(const unsigned char* src0, const unsigned char* src1, long frame_stride, int N, int H, int W, int C, int bgr,
                         const int* box, const int* frames_index, int n, int R, unsigned char* out, void* ws, void* stream);
/* crop + pad + resize + flip + crop + normalise in ONE resampling launch (behind the same table launch) that computes only the size x size
 * window: out fp32 (n, size, size, 4) NHWC4 with channels >= C zero, or with nchw != 0 (n, C, size, size).  Bit for bit
 * viai_frames_prep(viai_video_resize_u8(...)).  Refuses what viai_video_resize_u8 refuses, and size < 1, size > R, crop_x or crop_y < 0,
 * crop_x + size > R, crop_y + size > R.                                                                                                       */
int viai_video_prepare(const unsigned char* src0, const unsigned char* src1, long frame_stride, int N, int H, int W, int C, int bgr,
                       const int* box, const int* frames_index, int n, int R, int size, int crop_x, int crop_y, int flip, int nchw, float* out,
                       void* ws, void* stream);
/* viai_video_resize_u8 in plain C++, every pointer (box and frames_index too) in HOST memory; no workspace.  Same refusals.                   */
int viai_video_resize_u8_host(const unsigned char* src0, const unsigned char* src1, long frame_stride, int N, int H, int W, int C, int bgr,
                              const int* box, const int* frames_index, int n, int R, unsigned char* out);

/* ---- optical flow: TV-L1 from raw frames to the 8-bit flow maps (csrc/optical_flow.hip; additive to ABI v20) ----
 * The flow maps the video front end takes came with the reference's dataset as JPEG files; nothing in the reference computes them.  That they
 * are TV-L1 flow in the `dense_flow` encoding is an INFERENCE from Data_loaders/Image_preprocess.py (8-bit maps with "no motion" near 127, and a
 * motion threshold of 2 per frame, which is exactly what a still pixel, encoded as 128, contributes), not a record.  This is a statement of
 * TV-L1 of its own, not OpenCV's: parity with cv2's DualTVL1 is not claimed.
 *
 * ARITHMETIC.  fp32 throughout; only + - * / and sqrt, each correctly rounded and rounded ONCE (no contraction into fused multiply-adds, no
 * fast-math).  Sums written a + b + c are evaluated left to right.  The per-pixel functions exist once (csrc/viai_flow_rule.h) and both the
 * kernels and viai_optical_flow_host call them, so host and device agree bit for bit.  A fixed iteration count, no epsilon stop: no reductions,
 * no decisions on the host.
 *
 * 1 GREY.  g = (4899 R + 9617 G + 1868 B + 8192) >> 14 in int32, then to float (OpenCV's 8-bit BT.601, restated, not pinned).  C = 3 or 4
 *   interleaved channels (a fourth is ignored); bgr != 0 swaps R and B.  C = 1: the byte itself.
 * 2 PYRAMID.  Level 0 is the grey image, level k + 1 has ((h + 1) / 2, (w + 1) / 2) samples (integer division):
 *   L[k+1][y][x] = the 5 x 5 binomial at (2 y, 2 x) of level k, indices clamped to the image (replicated border).  ROWS FIRST: on each of the rows
 *   2 y - 2 .. 2 y + 2, r = 0.0625 a + 0.25 b + 0.375 c + 0.25 d + 0.0625 e over the columns 2 x - 2 .. 2 x + 2, the five products summed left
 *   to right; THEN the same expression over the five row results, top to bottom.  The number of levels is the largest S <= scales for which the
 *   coarsest level has both sides >= 16, and at least 1 (viai_optical_flow_levels).
 * 3 PER LEVEL, coarse to fine.  At the coarsest level u = v = 0.  p11 = p12 = p21 = p22 = 0 at the start of every level; they persist across the
 *   level's warps.  I1x[y][x] = 0.5 (I1[y][min(x + 1, w - 1)] - I1[y][max(x - 1, 0)]), I1y alike along y; I1 is frame t + 1.
 *   BILINEAR(A, cx, cy) on an h x w plane: cx is clamped to [0, w - 1] with `!(cx >= 0) ? 0 : cx > w - 1 ? w - 1 : cx` (a NaN lands on 0) BEFORE
 *   the floor; x0 = floor(cx), x1 = min(x0 + 1, w - 1), ax = cx - x0; y alike; the value is
 *   (1 - ay) ((1 - ax) A[y0][x0] + ax A[y0][x1]) + ay ((1 - ax) A[y1][x0] + ax A[y1][x1]).  No address is ever formed from an unclamped value.
 *   Going to a finer level: u_f[y][x] = 2 BILINEAR(u_c, (x + 0.5) / 2 - 0.5, (y + 0.5) / 2 - 0.5), v alike.
 * 4 PER WARP.  I1w, I1wx, I1wy = BILINEAR of I1, I1x, I1y at (x + u, y + v).  grad = I1wx I1wx + I1wy I1wy.
 *   rho_c = I1w - I1wx u - I1wy v - I0.
 * 5 PER ITERATION, `iterations` times per warp, lt = lam theta, taut = tau / theta:
 *   rho = rho_c + I1wx u + I1wy v.  d = lt I1wx when rho < -(lt grad); d = -(lt I1wx) when rho > lt grad; otherwise d = (-rho / grad) I1wx when
 *   grad > 1e-10, and 0 when not.  e alike with I1wy.
 *   u = (u + d) + theta (dx(p11) + dy(p12)), v = (v + e) + theta (dx(p21) + dy(p22)), with the backward differences
 *   dx(p)[x] = p[0] in the first column, -p[w - 2] in the last, p[x] - p[x - 1] between, and 0 when w == 1; dy alike over rows.
 *   Then, from the NEW u: ux = u[x + 1] - u[x], 0 in the last column; uy = u[y + 1] - u[y], 0 in the last row;
 *   den = 1 + taut sqrt(ux ux + uy uy); p11 = (p11 + taut ux) / den, p12 = (p12 + taut uy) / den.  p21, p22 the same from v.
 * 6 OUTPUT.  flow (N - 1, 2, H, W) fp32, pixels per frame at the input's resolution, map i = frame i -> frame i + 1, channel 0 = u (along x).
 *   ENCODING q = f < -bound ? 0 : f > bound ? 255 : rint(255 (f + bound) / (2 bound)), round half to even, the sum, the product, 2 bound and the
 *   quotient rounded once each; a NaN encodes as 0.  A still pixel is 127.5 -> 128.  pad_last != 0 writes the last map once more, so N frames
 *   give N maps.
 *
 * THE ITERATION KERNEL runs k <= VIAI_FLOW_MAX_ITERS_PER_LAUNCH iterations per launch: a block owns a VIAI_FLOW_TILE_H x VIAI_FLOW_TILE_W tile,
 * stages u, v and the four p of the tile plus a halo of k pixels (cut at the image) in LDS and recomputes the halo; halo pixels outside the image
 * are neither computed nor read.  A recomputed value runs the same operations on the same inputs, so THE RESULT DOES NOT DEPEND ON
 * iters_per_launch, nor on the remainder launch when it does not divide `iterations`.  Launches read one copy of the state and write the other.
 * No atomics, no cooperative launch, no waiting between blocks, no host synchronisation, nothing allocated; pair = grid z in every launch.   */
#define VIAI_FLOW_TILE_W 32
#define VIAI_FLOW_TILE_H 32
#define VIAI_FLOW_MAX_ITERS_PER_LAUNCH 8
#define VIAI_FLOW_ITERS_PER_LAUNCH 8 /* the default of the Python wrapper (DESIGN.md 11.2o has the measurement behind it) */
/* levels the pyramid of an H x W frame gets for `scales`; 0 for refused arguments.  Host arithmetic.                                          */
int viai_optical_flow_levels(int H, int W, int scales);
/* bytes of workspace for `pairs` pairs (pairs + 1 frames): the pyramids, two copies of the six evolving planes and the four constants of a
 * warp, 4 bytes x ((pairs + 1) x pyramid + 16 pairs H W).  0 for refused arguments (pairs < 1 or > 65535).  Host arithmetic.                 */
long viai_optical_flow_ws_bytes(int pairs, int H, int W, int scales);
/* launches of one viai_optical_flow call: 1 (grey) + S - 1 (pyramid) + S warps (1 + ceil(iterations / iters_per_launch)) + S - 1 (up-sampling)
 * + 1 (store); it does not depend on N.  0 for refused arguments.                                                                             */
int viai_optical_flow_launches(int H, int W, int scales, int warps, int iterations, int iters_per_launch);
/* frames (N, H, W, C) uint8 in DEVICE memory, frame f at frames + f frame_stride -> flow (N - 1, 2, H, W) fp32, DEVICE memory.  ws:
 * viai_optical_flow_ws_bytes(N - 1, H, W, scales) bytes of device memory, 4-byte aligned, overwritten.
 * Refuses with hipErrorInvalidValue before any launch: a NULL pointer; N < 2 or N - 1 > 65535; H or W < 1 or >= 2^15; C not 1, 3 or 4;
 * frame_stride < H W C; scales, warps or iterations < 1; iters_per_launch outside 1 .. 8; tau, lam or theta non-positive or NaN.            */
int viai_optical_flow(const unsigned char* frames, long frame_stride, int N, int H, int W, int C, int bgr, float tau, float lam, float theta,
                      int scales, int warps, int iterations, int iters_per_launch, float* flow, void* ws, void* stream);
/* the same rule in plain C++, every pointer in HOST memory, no workspace, no GPU.  Same refusals (iters_per_launch is checked and otherwise
 * has no effect, as on the device).                                                                                                           */
int viai_optical_flow_host(const unsigned char* frames, long frame_stride, int N, int H, int W, int C, int bgr, float tau, float lam, float theta,
                           int scales, int warps, int iterations, int iters_per_launch, float* flow);
/* flow (pairs, 2, H, W) fp32 -> flow_x, flow_y (pairs + (pad_last != 0), H, W) uint8, DEVICE memory, one launch.  Refuses before the launch: a
 * NULL pointer; pairs < 1 or > 65534; H or W < 1 or >= 2^15; a non-positive or NaN bound.                                                    */
int viai_flow_encode_u8(const float* flow, int pairs, int H, int W, float bound, int pad_last, unsigned char* flow_x, unsigned char* flow_y,
                        void* stream);
/* the same in plain C++ on HOST pointers.  Same refusals.                                                                                     */
int viai_flow_encode_u8_host(const float* flow, int pairs, int H, int W, float bound, int pad_last, unsigned char* flow_x,
                             unsigned char* flow_y);

/* ---- WAV in, WAV out: PCM decode, encode and in-place patching (csrc/wav_io.hip; additive to ABI v20) ----
 * The data chunk of a WAV file is `frames` FRAMES of `channels` interleaved little-endian samples, 1 <= channels <= 8; a waveform is planar fp32,
 * channel c at wav + c stride.  The per-sample arithmetic exists once, in csrc/viai_pcm_rule.h, for kernels and host mirrors: the same bits.
 *   DECODE   U8 (b - 128) / 128; S16 v / 2^15; S24 three bytes sign-extended, v / 2^23; S32 (float)v rounded to nearest even, then 2^-31;
 *            F32 the bits, non-finite values included; F64 the C cast to float.  mono: ((x0 + x1) + ...) + x_{C-1} in fp32 in channel order, then
 *            one IEEE fp32 division by (float)C.
 *   ENCODE   integer formats rint(x 2^(bits-1)), ties to even, clamped to the format's range in float before the conversion (x >= 1 is the
 *            maximum, never a wrap); U8 rint(128 x) + 128 clamped to 0 .. 255; a non-finite x is 0 (128 for U8); F32 the bits; F64 the exact
 *            widening.
 *   NORMALISED ENCODE (S16 only; `save_wav` of utils/audio.py:19-21)  peak = max |x| over the finite samples of all channels; scale = 3276700.0f
 *            when (double)peak <= 0.01, else the fp32 quotient 32767.0f / peak; the sample is (int16) trunc(fl32(x scale)); a non-finite sample
 *            is 0 and does not enter the peak.
 * One block owns VIAI_PCM_TILE frames: a multiple of 16, so a tile starts 16-byte aligned in the byte stream for every frame size (9-byte
 * S24 x 3 frames included), and at most 64 KiB of bytes (8 channels of F64).                                                                   */
enum { VIAI_PCM_U8 = 0, VIAI_PCM_S16 = 1, VIAI_PCM_S24 = 2, VIAI_PCM_S32 = 3, VIAI_PCM_F32 = 4, VIAI_PCM_F64 = 5 };
#define VIAI_PCM_TILE 1024
/* src: frames x channels samples, DEVICE memory, 16-byte aligned -> out (channels, frames) fp32, channel c at out + c out_stride, or (1, frames)
 * when mono != 0.  ONE launch: a block brings its tile into LDS with 16-byte loads (the tail of the last tile byte by byte), lanes read their
 * samples from LDS and write four frames of a plane with one 16-byte store where the address allows it.  frames = 0: nothing is launched.
 * Every viai_pcm_* call refuses with hipErrorInvalidValue before any launch, and so also on a machine without a device: an unknown format;
 * channels outside 1 .. 8; frames < 0 or more than 2^31 - 1 tiles; a stride < frames; a NULL pointer; src / dst not 16-byte or a waveform not
 * 4-byte aligned (device calls only); normalize with a format other than S16.                                                                 */
int viai_pcm_decode(const unsigned char* src, int fmt, int channels, long frames, int mono, float* out, long out_stride, void* stream);
/* bytes of workspace of a normalised encode: one fp32 per tile.  Host arithmetic; 0 for frames < 0.                                           */
long viai_pcm_ws_bytes(long frames);
/* max |x| over the finite samples of every tile -> ws[tile] (fp32), one launch, one block per tile.  A maximum does not depend on order.      */
int viai_pcm_peak(const float* wav, long stride, int channels, long frames, float* ws, void* stream);
/* wav planar fp32 -> dst, frames x channels samples.  ONE launch without normalize (ws may be NULL); with it viai_pcm_peak runs first and every
 * block of the encode launch reduces the partials itself: no atomic, no synchronisation, no host copy.  The transpose goes through LDS, dst
 * is written with 16-byte stores (the tail byte by byte).                                                                                    */
int viai_pcm_encode(const float* wav, long stride, int channels, long frames, int fmt, int normalize, unsigned char* dst, void* ws, void* stream);
/* dst already holds the file's data bytes.  Encodes, plain rule, ONLY samples [start[c][k], start[c][k] + length[c][k]) of channel c, clamped to
 * [0, frames), for k < min(count[c], K); count (channels,), start and length (channels, K) int32 in DEVICE memory, as viai_gap_detect leaves
 * them.  Every store is as wide as one sample or narrower: no other byte of dst is read or written.  K < 1 is refused.                         */
int viai_pcm_patch(const float* wav, long stride, int channels, long frames, int fmt, const int* count, const int* start, const int* length, int K,
                   unsigned char* dst, void* stream);
/* the same three in plain C++ from the same rule header, every pointer in HOST memory, no workspace, no alignment rule.  Same refusals.        */
int viai_pcm_decode_host(const unsigned char* src, int fmt, int channels, long frames, int mono, float* out, long out_stride);
int viai_pcm_encode_host(const float* wav, long stride, int channels, long frames, int fmt, int normalize, unsigned char* dst);
int viai_pcm_patch_host(const float* wav, long stride, int channels, long frames, int fmt, const int* count, const int* start, const int* length,
                        int K, unsigned char* dst);

/* ---- vocoder data preparation: waveform -> (signal, aligned row) per chunk (additive to ABI v20, csrc/preprocess.hip) ----
 * `_process_utterance` of utils/librivox.py:44-117 behind the file decode.  A file wav (n_samples floats) is cut into n_chunks chunks
 * [chunk_off[c], chunk_off[c] + chunk_len[c]) -- int32 arrays in DEVICE memory; the part of a chunk outside the file is ignored.  Each call is one
 * launch for all chunks.  Rescaling: with amax != NULL -- a DEVICE float, max |wav| from viai_absmax -- every sample is taken as
 * x / *amax * rescaling_max, an fp32 division and an fp32 multiplication each rounded on its own (numpy's float32 arithmetic, librivox.py:48-49);
 * with amax == NULL samples are taken as they are.  mu = quantize_channels - 1.  Both refuse on the host, before any HIP call and so also on a
 * machine without a device: a null pointer (amax excepted), n_chunks < 1, n_samples < 1 or above INT32_MAX, mu < 1; trim_bounds also thr < 0;
 * pack also hop < 1, hop > fft, an unknown mode, max_len < 1, a capacity < 1 or above INT32_MAX, n_chunks > 65535.
 *
 * The silence trim (utils/audio.py:56-67 as librivox.py:66-73 calls it): with class(i) the mu-law class of sample i of the chunk -- computed on the
 * fly by the device function of viai_mulaw_quantize, no class array is written -- and active(i) = |class(i) - silence_class| > thr,
 *     bounds[c][0] = the first active i,                 chunk_len[c] if there is none
 *     bounds[c][1] = the last active i among i >= 2,     -1 if there is none        (the reference's backward loop never looks at i = 0, 1)
 * One block per chunk, integer min / max only: the same bits on every run.                                                                    */
int viai_utt_trim_bounds(const float* wav, long n_samples, const int* chunk_off, const int* chunk_len, int n_chunks, const float* amax,
                         float rescaling_max, int mu, int thr, int silence_class, int* bounds, void* stream);
/* Given bounds[c] = (start, end), END EXCLUSIVE as in wav[start:end] (the sample at `end` is dropped, as the reference drops it), T = end - start:
 *   rows[row_off[c] + i]      = sample start + i of the chunk, rescaled, i < T: what the mel front end reads.  With rows 16-byte aligned and
 *                               row_off[c] % 4 == 0 a row starts 16-byte aligned (viai_stft_mel_route decides by the pointer's alignment) and is
 *                               written with vector stores.
 *   signal[sig_off[c] + j]    j < N hop, N = lws_num_frames(T, fft, hop): l = fft - hop pad values, the T samples, pad values up to N hop
 *                               (lws_pad_lr and the cut of librivox.py:92-102) in the form `mode` names:
 *       VIAI_UTT_MULAW_QUANTIZE  int32 classes of viai_mulaw_quantize, pad mu / 2;
 *       VIAI_UTT_MULAW           floats y = sign(x) log1p(mu |x|) / log1p(mu), the same device function before its class step, pad 0.0;
 *       VIAI_UTT_RAW             the floats themselves (with amax == NULL: bit for bit), pad 0.0.
 * row_off, sig_off: int32 in device memory, in elements; rows_cap / signal_cap: elements the two buffers hold, no store goes beyond them.
 * A chunk with end <= start writes nothing.  max_len (the longest chunk) sizes the grid only.                                                */
enum { VIAI_UTT_MULAW_QUANTIZE = 0, VIAI_UTT_MULAW = 1, VIAI_UTT_RAW = 2 };
int viai_utt_pack(const float* wav, long n_samples, const int* chunk_off, const int* chunk_len, const int* bounds, int n_chunks, int max_len,
                  const float* amax, float rescaling_max, int mode, int mu, int fft, int hop, const int* row_off, float* rows, long rows_cap,
                  const int* sig_off, void* signal, long signal_cap, void* stream);
/* WaveNet training batches (csrc/vocoder_batch.hip, additive to ABI v20): `collate_fn` of Data_loaders/data_loader_utils.py:209-319 behind its
 * crop draw -- crop on the frame grid, zero padding to the batch's longest row, targets, class / one-hot / float inputs and the mel transposed,
 * in ONE launch for the whole batch.  Row b is a pair of viai_utt_pack's making, read where it lies:
 *   sig_ptr[b]  its signal, int32 classes (mode VIAI_UTT_MULAW_QUANTIZE) or floats (VIAI_UTT_MULAW, VIAI_UTT_RAW), 4-byte aligned
 *   mel_ptr[b]  its mel, (N, D) fp32 row-major; mel_ptr == NULL (with c == NULL): no local conditioning
 *   start[b], frames[b]   the crop: frames [start, start + frames) of the mel, samples [start hop, (start + frames) hop) of the signal.
 *                         The four tables are arrays of B entries in DEVICE memory; frames[b] is clamped to [0, L_out], start[b] to >= 0.
 * With t < T_out = L_out * hop, len = frames[b] * hop and s = the row's signal from sample start[b] * hop on:
 *   mode 0:     y [B][T_out] int64 (the (B, T, 1) targets) = s[t], 0 for t >= len;  classes [B][T_out] int32, the same numbers (NULL: not
 *               written);  x [B][K][T_out] fp32 (NULL: not written) = 1.0 where s[t] == k, else 0.0 -- a column at t >= len, or of a class
 *               outside [0, K), is all zero.  No store address depends on a class.
 *   modes 1, 2: y is a float buffer [B][T_out] = the bits of s[t], 0.0 for t >= len: the (B, 1, T) input and the (B, T, 1) target of the
 *               reference hold the same numbers in the same order, so one buffer is both.  classes and x are not touched.
 *   c [B][D][L_out] fp32 = mel[start[b] + f][d] at [b][d][f], 0.0 for f >= frames[b].
 * Nothing is read past sample (start + frames) * hop resp. frame start + frames of a row, nothing is written outside the extents above.
 * 16-byte loads for a row when hop % 4 == 0 and its first kept sample is 16-byte aligned, 16-byte stores when every output base is 16-byte
 * aligned and T_out % 4 == 0; element by element otherwise, same results.
 * Refused on the host before any HIP call (so also without a device): a NULL sig_ptr, start, frames or y; B < 1 or > 65535; hop < 1; an unknown
 * mode; K < 2 in mode 0; K % 4 != 0 with x given; D < 1 with mel_ptr given; mel_ptr without c or c without mel_ptr; T_out < hop,
 * T_out % hop != 0, L_out * hop != T_out, T_out > INT32_MAX; an output pointer that is not aligned to its element.                          */
int viai_voc_collate(const void* const* sig_ptr, const float* const* mel_ptr, const int* start, const int* frames, int B, int hop, int D, int mode,
                     int K, long T_out, int L_out, long long* y, int* classes, float* x, float* c, void* stream);

/* Incremental synthesis as ONE persistent launch (ABI v16, csrc/wavenet_pipe.hip): a weight-stationary pipeline for the reference-size
 * network (24 layers, 512 residual / 512 gate / 256 skip channels, 80 conditioning channels, 30 outputs, no global conditioning).  Every
 * stage owns compute units (10 per layer, 4 + 4 + 1 for the head) and keeps its weights in registers / LDS; the streams travel round the
 * stages as tokens of 8-byte {tag, value} granules, so up to B stages work at once where the chain form (viai_wavenet_synth_run) has one.
 * Same time steps, same folded weights (layers[].w_stage / b_stage), fp32, fixed summation order; replaces the per-step loop of
 * wavenet.py:322-357 for this configuration.
 *   viai_wn_pipe_ok            1 if `s` is that configuration (mixture-of-logistics output: 0 for a categorical descriptor) with 1 .. 32 streams and
 *                              the device has >= 256 compute units (all blocks must be resident)
 *   viai_wn_pipe_image_floats  sizes of the five weight images the HOST packs (viai_amd.wavenet._pipe_images): 0 wreg [24][10][8][156][64],
 *                              1 wlds [24][10][130][260], 2 bias [24][10][136], 3 head_w [544][256], 4 head_b [544], 5 wcond [24][10][64][80]
 *   viai_wn_pipe_token_granules  8-byte granules of the token rings for B streams (dil: the 24 dilations)
 *   viai_wn_pipe_run           time steps [t0, t0 + n_steps) of every stream.  tok: the rings, ZERO before t0 == 0 and carried over between
 *                              calls; err: 4 zeroed uint32, err[0] != 0 afterwards = failure (1: a wait timed out at stage / stream / t =
 *                              err[1..3]) -- the caller must check it after synchronising.                                                 */
int viai_wn_pipe_ok(const viai_wn_synth* s);
/* debug aid (tools/wn_pipe_stamps.py): later viai_wn_pipe_run calls record wall-clock stamps (100 MHz) of time step t on compute unit 0 of every stage
 * into buf, 2 x [27 stages][8 streams][8] uint64 (wall clock, then shader cycles; 0 wait begins / 1 x part complete / 2 z part complete / 3 published / 4 .. 7 inside a layer
 * stage: residual rows done, past barrier 1, gate rows done, past barrier 2); buf = NULL switches it off */
int viai_wn_pipe_profile(void* buf, int t);
long viai_wn_pipe_image_floats(int which);
long viai_wn_pipe_token_granules(int B, const int* dil);
int viai_wn_pipe_run(const viai_wn_synth* s, const float* wreg, const float* wcond, const float* wlds, const float* bias, const float* head_w, const float* head_b,
                     void* tok, unsigned* err, int t0, int n_steps, void* stream);

/* ------------------------------------------------------------ mask / optimizer
 * s_in = s * mask, mask (N, T) broadcast over frequency (the missing
 * AudioModel.set_inputs; figure misc/pipeline2.png)                             */
int viai_mask_mul(const float* s, const float* mask, float* out, int N, int F, int T, void* stream);
/* the loss scalars an iteration reports (train_whole_sync.py:85-112 reads them through get_loss_items / get_current_errors), from the
 * device scalars the loss kernels left: out[0] = 0.5 (d_fake + d_real), out[1] = g_gan + lambda_l1 l1 (+ lambda_c contrast), out[2] = g_gan,
 * out[3] = l1, out[4] = d_real, out[5] = contrast (only when contrast != NULL).  One launch instead of ten one-element kernels.     */
int viai_step_scalars(const float* d_real, const float* d_fake, const float* g_gan, const float* l1, const float* contrast,
                      float lambda_l1, float lambda_c, float* out, void* stream);
/* torch.optim.Adam step on a flat fp32 arena (optimizer_G / optimizer_D,
 * utils/util.py:149-150).  `state` is 4 device doubles {step, lr, beta1^t, beta2^t}
 * (initialise to {0, lr, 1, 1}) advanced ON DEVICE so that the launch is
 * replayable inside a hipGraph.                                                  */
int viai_adam_step(float* p, const float* g, float* m, float* v, long n, double* state,
                   double beta1, double beta2, double eps, float grad_scale, void* stream);

/* out[c] (+)= sum over rows of x[M][C] (bias gradients); part: scratch of
 * viai_colsum_blocks(M, C) * C floats                                            */
int viai_colsum_blocks(long M, int C);
int viai_colsum(const float* x, long M, int C, float* part, float* out, int accumulate, void* stream);

/* Debug aid for the f16x2 conv arithmetic (operands are pre-scaled by powers of two and SATURATE beyond the fp16 range:
 * activations above 65504 / 16 ~ 4094, weights above 65504 / 256 ~ 255): counts[0] += #{|x_i| > limit},
 * counts[1] = max(counts[1], bit pattern of max |x_i|), counts[2] += #{non-finite x_i}.  counts: 3 zero-initialised uint32. */
int viai_range_count(const float* x, long n, float limit, unsigned* counts, void* stream);

/* y = a*x + y (flat); used for gradient accumulation on arenas */
int viai_axpy(float a, const float* x, float* y, long n, void* stream);

/* ----------------------------------------------------------------- audio front
 * melspectrogram(y) of utils/audio.py:70-75 (lws STFT -> |.| -> mel -> dB -> [0,1])
 * fused with the inpainting mask.  basis_t: [fft/2+1][n_mels] (TRANSPOSED mel basis); window: [fft]; mask: [B][frames] or NULL.
 * wav: [B][n_samples]; mel out: [B][n_mels][frames] (== NHWC with C = 1).        */
int viai_stft_mel(const float* wav, const float* window, const float* basis_t, const float* mask,
                  float* mel, int B, int n_samples, int fft, int hop, int n_mels, int frames,
                  float min_level_db, float ref_level_db, void* stream);
/* The same stage (utils/audio.py:70-75) on the frame-batched kernel, fft = 1024 (ABI v4): eight frames per block, two real frames per
 * complex radix-4 FFT, and a BANDED mel basis -- the caller states the support of each band of `basis_t`:
 * basis_t[k][m] == 0 outside k in [band_lo[m], band_lo[m] + band_cnt[m])  (librosa.filters.mel rows are triangles a few bins wide;
 * a dense basis is expressed by band_lo = 0, band_cnt = fft/2 + 1).  Same outputs as viai_stft_mel.                                  */
int viai_stft_mel_banded(const float* wav, const float* window, const float* basis_t, const int* band_lo, const int* band_cnt,
                         const float* mask, float* mel, int B, int n_samples, int fft, int hop, int n_mels, int frames,
                         float min_level_db, float ref_level_db, void* stream);
/* Which kernel family a front-end call of this shape runs on, without a launch (host code only; measurement aid, no reference
 * counterpart).  fft = 1024 answers for viai_stft_mel_banded, which chooses by shape: "r512" (one real frame per wave as a 512-point
 * complex FFT: n_mels <= 256, a hop that is a multiple of 8, an even n_samples and a `wav` pointer aligned to 8 bytes -- wav_aligned8 != 0),
 * else "wave" (two real frames per wave as one 1024-point FFT: n_mels <= 1024, a hop that is a multiple of 8), else "banded" (the frame-batched
 * kernel: any hop, any band count; the two wave kernels were measured wrong in the frames that cross a clip's start at hops 254, 255, 257).  fft = 512 / 2048 answer
 * "dense": only viai_stft_mel serves them, on its one kernel (one frame per block, every bin of every band), which it also runs for
 * fft = 1024.  The launch decides by the same function.  Whether the band weights are held in LDS depends on the sum of band_cnt,
 * which is device data (r512: <= 1024, wave: <= 2048; else they are read from global memory): not part of the answer.
 * family receives the NUL-terminated name (truncated to cap); returns 1, or 0 with an empty name where the entry point refuses.    */
int viai_stft_mel_route(int n_samples, int fft, int hop, int n_mels, int wav_aligned8, char* family, int cap);
/* The same stage on clips of DIFFERENT lengths in one call (fft = 1024; additive to ABI v20, no reference counterpart: the reference
 * computes one mel per call).  Row r is the row_len[r] samples at wav + row_off[r]; rows may be packed back to back, leave gaps or
 * overlap.  Every row is computed as a one-clip call of viai_stft_mel_banded on its own samples computes it, bit for bit: the zero padding
 * on either side of a row is zero whatever lies next to it, its frame tiles start at its own frame 0, and it runs on the kernel family
 * viai_stft_mel_route names for (row_len[r], fft, hop, n_mels, alignment of wav + row_off[r]).
 *
 * viai_stft_mel_ragged_plan -- host code only, no HIP call, no device needed -- turns row offsets and lengths into the tables:
 *   in    row_off   [n_rows]      int64, samples from `wav`, >= 0
 *         row_len   [n_rows]      int32, samples, 1 .. 2^29 - 1
 *         base_aligned8           whether `wav` itself will be 8-byte aligned (row r is then aligned iff row_off[r] is even; with a base
 *                                 4 bytes off, iff it is odd)
 *   out   row_frames [n_rows]     frames of row r = lws_num_frames(row_len[r], fft, hop)
 *         frame_off  [n_rows + 1] prefix sum of row_frames: row r owns output columns frame_off[r] .. frame_off[r + 1]
 *         row_family [n_rows]     VIAI_STFT_R512 / _WAVE / _BANDED
 *         items      [n][2]       int32 pairs (row, first frame of a tile), grouped by family in the order r512, wave, banded; inside a
 *                                 family in row order, a row's tiles in frame order from frame 0.  A tile is 32 frames on r512 and wave,
 *                                 8 on banded; the last tile of a row may be short.  Every (row, frame) is in exactly one tile.
 *         family_items [3]        items of r512, wave, banded (their sum is n)
 *   Any out pointer may be NULL.  Returns 0 when `items` was filled; the item count n (> 0) when items == NULL or item_cap < n (the
 *   other outputs are written all the same: call with items = NULL to size the list); -1 where it refuses: n_rows < 1, a length
 *   outside 1 .. 2^29 - 1, a negative offset, fft != 1024, a hop or n_mels viai_stft_mel_route refuses, more than 2^31 - 1 frames or
 *   2^30 - 1 items in all.
 *
 * viai_stft_mel_ragged runs them: row_off, row_len, row_frames, frame_off and items are DEVICE copies of the arrays above (row_family
 * stays on the host), family_items is the HOST array.  At most one launch per family present, persistent blocks over the family's items.
 *   out, time_major == 0:  row r is a contiguous [n_mels][row_frames[r]] block at out + n_mels * frame_off[r]
 *        time_major != 0:  one [frame_off[n_rows]][n_mels] array, row r at its rows frame_off[r] .. frame_off[r + 1]
 *   Either way the call writes the n_mels * frame_off[n_rows] floats from `out` on and nothing else.
 *   mask: NULL, or one float per output column, [frame_off[n_rows]]: column frame_off[r] + f scales frame f of row r (an fp32 product).
 * Returns hipErrorInvalidValue before any launch on a NULL table or operand (mask excepted), n_rows < 1, no item, fft != 1024, or a
 * family with items on a shape its kernel does not take.  The tables are trusted: hand in what the plan wrote.                      */
enum { VIAI_STFT_R512 = 1, VIAI_STFT_WAVE = 2, VIAI_STFT_BANDED = 3 };
long viai_stft_mel_ragged_plan(const long long* row_off, const int* row_len, int n_rows, int fft, int hop, int n_mels, int base_aligned8,
                               int* row_frames, int* frame_off, int* row_family, int* items, long item_cap, int* family_items);
int viai_stft_mel_ragged(const float* wav, const long long* row_off, const int* row_len, const int* row_frames, const int* frame_off,
                         const int* items, const int* family_items, int n_rows, const float* window, const float* basis_t,
                         const int* band_lo, const int* band_cnt, const float* mask, float* out, int fft, int hop, int n_mels,
                         int time_major, float min_level_db, float ref_level_db, void* stream);

/* -------------------------------------------------- callers either side of the path
 * Batch assembly on the device, Data_loaders/audio_loader.py:185-245: frames uint8 [n][S][S][C] (RGB or
 * (flow_x, flow_y), already resized to S x S) -> float NHWC4 [n][size][size][4] = (px - 127) / 128 after the
 * left-right flip and the crop of rows [crop_x, +size) x columns [crop_y, +size).                           */
int viai_frames_prep(const unsigned char* frames, float* out, long n, int S, int C, int size,
                     int crop_x, int crop_y, int flip, void* stream);
/* audio_loader.py:471-475,508,523: clip b = mel frames [3 + 4*start[b], +L) of c [T_total][D] -> c_out [B][D][L]
 * (channel first), and samples [(3 + 4*start[b]) * hop, +L*hop) of x -> x_out [B][L*hop]; zero padded past the end. */
int viai_slice_clips(const float* c, const float* x, const int* start, float* c_out, float* x_out,
                     int B, int D, int L, int hop, long T_total, long samples, void* stream);
/* loss_functions.py:65-76 ExponentialMovingAverage.update on a flat buffer: shadow -= (1 - decay) * (shadow - x) */
int viai_ema_update(float* shadow, const float* x, long n, double decay, void* stream);
/* utils/audio.py:135-144: out = 10 ^ ((clip(S, 0, 1) * -min_level_db + min_level_db) / 20)  (_denormalize, _db_to_amp) */
int viai_mel_denorm_amp(const float* S, float* out, long n, float min_level_db, void* stream);
/* utils/util.py:99-121 L2retrieval: for caption i, ranks[i] = position of clip i in the ascending order of
 * |captions[i] - clips[j]|_2 over j, top1[i] = argmin_j; dist (optional) [n_captions][n_clips].             */
int viai_l2_ranks(const float* clips, const float* captions, int n_clips, int n_captions, int dim,
                  int* ranks, int* top1, float* dist, void* stream);

/* Fused pair: (conv + BatchNorm + activation) -> (3 x 3, stride 1, pad 1 conv or stride-1 transposed conv with ONE output channel).
 * Reference pairs: G.conv6_1 + conv6_1_bn + ReLU -> conv6_2 (New_Inpainting_Networks.py:85-88, 134 MB per tensor at the benchmark size)
 * and D.conv3 + norm3 + LeakyReLU -> conv4 (Discriminator_Networks.py:44-49).  Neither the front layer's post-activation tensor z nor the
 * Cout = 1 layer's data gradient dz is ever stored: the Cout = 1 kernels read the front layer's PRE-BatchNorm output y and apply
 * z = act_in(scale * y + shift) on load; the BatchNorm backward forms dz = conv_backward_data(du, w) -- nine float4 FMAs per element from
 * a register window of the one-channel du -- instead of reading it back twice.  `c` describes the Cout = 1 layer (C1 = the front layer's
 * channels: 32 .. 512, width a multiple of 16); wp = its packed image (viai_conv2d_pack_fwd); du = gradient of its PRE-activation output.
 *   fwd:    out = act(conv(z, w) + bias)
 *   wgrad:  dw (+)= conv_backward_weight(z, du);  ws: viai_conv2d_wgrad_ws_bytes(c)
 *   bn_bwd: the front layer's BatchNorm + activation backward (viai_bn_act_bwd_amax semantics: sums = {k0, k1}, dgamma, dbeta, dy, max |dy|);
 *           part: 2 * C1 * viai_pair_cout1_bn_bwd_blocks(c) floats                                                                          */
int viai_pair_cout1_ok(const viai_conv2d* c);
int viai_pair_cout1_bn_bwd_blocks(const viai_conv2d* c);
int viai_pair_cout1_fwd(const viai_conv2d* c, const float* y, const float* scale, const float* shift, int act_in,
                        const float* wp, const float* bias, float* out, int act, void* stream);
/* fwd through a per-pixel tensor of the nine tap products (ws: 9 * N * IH * IW floats): one grid-stride pass over y + a gather -- the form
 * wide front layers take (D.conv3 -> conv4, 512 channels), where a block of whole rows leaves too few pixels in flight (ABI 11)            */
int viai_pair_cout1_fwd_dots(const viai_conv2d* c, const float* y, const float* scale, const float* shift, int act_in,
                             const float* wp, const float* bias, float* ws, float* out, int act, void* stream);
int viai_pair_cout1_wgrad(const viai_conv2d* c, const float* y, const float* scale, const float* shift, int act_in,
                          const float* du, float* ws, float* dw, int accumulate, void* stream);
int viai_pair_cout1_bn_bwd(const viai_conv2d* c, const float* du, const float* wp, const float* y, const float* mean,
                           const float* invstd, const float* scale, const float* shift, int act_in, float* part, float* sums,
                           float* dgamma, float* dbeta, float* dy, int training, float* dy_amax, void* stream);

/* -------------------------------------------------- fused Cin = 1 conv + BatchNorm2d(train) + activation layer (ABI v5)
 * MelEncoder.conv1 + bn1 + LeakyReLU (Inpainting_Networks.py:55,71) and MelDiscriminator's first block (Discriminator_Networks.py:17-19,
 * 38-39): with 4 .. 9 taps and one input channel the convolution is cheaper to RECOMPUTE than its 32 / 64-channel output is to write
 * and read back, so the pre-BatchNorm tensor y never exists in memory (same arithmetic, same order as viai_conv2d_fwd + viai_bn_*):
 *   fwd(z = NULL): BatchNorm partials (layout of viai_conv2d_fwd's stat_part, geometry of viai_conv2d_stat_geom) -> viai_bn_finalize
 *   fwd(stat_part = NULL): z = act(scale * conv(x) + shift); z_amax (optional, zero-initialised device float) receives max |z|
 *   bwd: partial sums from (dz, recomputed y) -> sums = {k0, k1}, dgamma, dbeta;  dy only if a data gradient needs it in memory
 *        (`training` as in viai_bn_act_bwd; part: 2 * Cout * nblk floats, nblk from viai_conv2d_stat_geom)
 *   wgrad: dw (+)= sum dy * x with dy formed on the fly from dz, y and sums
 * w: the packed image of viai_conv2d_pack (= the torch layout for this kind).
 * x_mask (optional, (N, IW) floats): x is read as x[n][iy][ix] * x_mask[n][ix] -- the time mask of the inpainting step (s_in = s * mask,
 * the missing AudioModel.set_inputs; misc/pipeline2.png) applied where E.conv1 loads s, not in a pass of its own (ABI 8).           */
int viai_conv2d_cin1_bn_ok(const viai_conv2d* c);
int viai_conv2d_cin1_bn_fwd(const viai_conv2d* c, const float* x, const float* x_mask, const float* w, const float* bias, float* stat_part,
                            const float* scale, const float* shift, float* z, int act, float* z_amax, void* stream);
int viai_conv2d_cin1_bn_bwd(const viai_conv2d* c, const float* x, const float* x_mask, const float* w, const float* bias, const float* dz,
                            const float* mean, const float* invstd, const float* scale, const float* shift, float* part,
                            float* sums, float* dgamma, float* dbeta, float* dy, int act, int training, void* stream);
int viai_conv2d_cin1_bn_wgrad(const viai_conv2d* c, const float* x, const float* x_mask, const float* w, const float* bias, const float* dz,
                              const float* mean, const float* scale, const float* shift, const float* sums, float* ws,
                              float* dw, int accumulate, int act, void* stream);
/* dx straight from dz (dy formed per contributing output pixel): no dy tensor at all; needs bias == NULL */
int viai_conv2d_cin1_bn_dgrad(const viai_conv2d* c, const float* x, const float* x_mask, const float* w, const float* dz, const float* mean,
                              const float* scale, const float* shift, const float* sums, float* dx, int act, void* stream);

/* -------------------------------------------------- (ABI 13) pre-split activations and gradients: the P16 layout
 * Between a BatchNorm pass and the f16x2 conv kernels that consume its output nothing needs fp32: every consumer (the next layer's forward,
 * this layer's data gradient, the weight gradients on either side) splits each value into two fp16 terms, value * S = lead + rem, S a power
 * of two, while it stages the tile -- up to four times per tensor and step, 6 VALU per element pair each time, in kernels that rocprofv3
 * shows issue-bound (6 - 7 non-MFMA VALU per MFMA in the stride-2 and 32-channel families, profiles/r04_a_pmc_*.json).  A P16 tensor holds
 * the two terms instead of the fp32 value, in the SAME bytes: shape (N, H, W, C) "fp32", C % 32 == 0; per pixel and 32-channel group g the
 * 128 bytes at g * 128 are [32 x fp16 lead (64 B)][32 x fp16 rem (64 B)].  A consumer stages 16-byte PIECES (8 channels of one plane) where
 * it staged 16-byte channel quads: same addresses, no conversion, one 16-byte LDS store.
 * The scale S = 2^(14 - e), magnitude < 2^e, must be known BEFORE the pass that writes the planes, so it is derived from an a-priori BOUND
 * of the tensor (written to *amax for the consumers), not from its measured maximum:
 *   forward (training-mode statistics over m_stat samples):  |act(gamma xhat + beta)| <= |gamma| sqrt(m_stat - 1) + |beta|   (Samuelson)
 *   backward: |dy| <= |scale| max|dpre| + |k1| sqrt(M - 1) / invstd + |k0| per channel, max|dpre| reduced with the sums
 * fp16 keeps 11 bits at every magnitude down to 2^-14 S^-1, so values 2^10 below the bound still carry 22 bits (tests/test_p16_gpu.py).
 * The arithmetic is that of the fp32-input kernels handed the same *amax, bit for bit.
 * Reference semantics: the tensors between nn.BatchNorm2d / LeakyReLU and the next nn.Conv2d (Discriminator_Networks.py:38-46,
 * New_Inpainting_Networks.py:31-37) -- an internal format; the module API keeps returning fp32.                                       */
#define VIAI_P16_DY 1              /* viai_conv2d_wgrad_f16_p16 flags: dy is P16 (scale from *dy_amax) */
#define VIAI_P16_X 2               /*                                  x is P16 (scale from *x_amax; no x2) */
#define VIAI_P16_OK_FWD_X 1        /* viai_conv2d_p16_ok mask: the forward kernel takes a P16 x */
#define VIAI_P16_OK_DGRAD_DY 2     /*                          the data-gradient kernel takes a P16 dy */
#define VIAI_P16_OK_WGRAD_DY 4     /*                          the weight-gradient kernel takes a P16 dy */
#define VIAI_P16_OK_WGRAD_X 8      /*                          ... and a P16 x */
#define VIAI_P16_OK_FWD_LIN 16     /*                          the P16 forward writes its BatchNorm partials per 128 CONSECUTIVE pixels
                                                                (viai_bn_finalize with rows = 128, nblk = M / 128), whatever viai_conv2d_stat_geom says of the fp32-input launch */
int viai_conv2d_p16_ok(const viai_conv2d* c);
/* z (P16) = act(scale * y + shift); gamma / beta (NULL = 1 / 0) and m_stat give the bound; *z_amax receives it.  act: none / ReLU / LeakyReLU */
int viai_bn_act_fwd_p16(const float* y, const float* scale, const float* shift, const float* gamma, const float* beta, long m_stat,
                        float* z, long M, int C, int act, float slope, float* z_amax, void* stream);
/* viai_bn_add_act_fwd_amax (the residual join of networks/ResNet.py:49-53) writing z twice: fp32 (z, exact maximum to *z_amax: the next join's residual, the
 * backward's mask) and P16 (z_p16, bound |gamma| sqrt(m_stat - 1) + |beta| + *res_amax to *p_amax: what the next block's conv1 stages).  C / 4 a power of two <= 256 */
int viai_bn_add_act_fwd_twin(const float* y, const float* scale, const float* shift, const float* gamma, const float* beta, long m_stat,
                             const float* res, const float* res_amax, float* z, float* z_p16, long M, int C, int act, float slope,
                             float* z_amax, float* p_amax, void* stream);
/* viai_bn_act_maxpool_fwd (3 x 3 / stride 2 / pad 1 only) writing the pooled tensor twice: fp32 (out, exact maximum to *out_amax) and P16 (out_p16, bound to
 * *p_amax) -- the stem of networks/Image_Embedding.py:20-23 in front of the first BasicBlock.  C % 32 == 0 */
int viai_bn_act_maxpool_fwd_twin(const float* y, const float* scale, const float* shift, const float* gamma, const float* beta, long m_stat,
                                 float* out, float* out_p16, unsigned char* idx, int N, int IH, int IW, int C, int k, int s, int p, int act, float slope,
                                 float* out_amax, float* p_amax, void* stream);
/* viai_bn_act_bilinear_fwd_amax with the resized tensor written as P16 */
int viai_bn_act_bilinear_fwd_p16(const float* y, const float* scale, const float* shift, const float* gamma, const float* beta, long m_stat,
                                 float* out, int N, int IH, int IW, int OH, int OW, int C, int act, float slope, float* z_amax, void* stream);
/* the apply pass of the fused Cin = 1 layer (viai_conv2d_cin1_bn_fwd with z != NULL) writing z as P16 */
int viai_conv2d_cin1_bn_fwd_p16(const viai_conv2d* c, const float* x, const float* x_mask, const float* w, const float* bias,
                                const float* scale, const float* shift, const float* gamma, const float* beta, long m_stat,
                                float* z, int act, float* z_amax, void* stream);
/* viai_pair_cout1_bn_bwd with dy written as P16 (part: 3 * C * blocks floats, sums: 3 * C floats) */
int viai_pair_cout1_bn_bwd_p16(const viai_conv2d* c, const float* du, const float* wp, const float* y, const float* mean,
                               const float* invstd, const float* scale, const float* shift, int act_in, float* part, float* sums,
                               float* dgamma, float* dbeta, float* dy, int training, float* dy_amax, void* stream);
/* viai_bn_act_bwd_amax with dy written as P16; part: 3 * C * viai_bn_bwd_blocks(M, C) floats, sums: 3 * C floats; *amax receives the bound */
int viai_bn_act_bwd_p16(const float* dz, const float* y, const float* mean, const float* invstd,
                        const float* scale, const float* shift, float* part, float* sums,
                        float* dgamma, float* dbeta, float* dy, long M, int C, int act, float slope,
                        int training, float* amax, void* stream);
/* (ABI 15) the same with the fp32 tensor written beside the planes (dy32: M x C floats, the values of viai_bn_act_bwd_amax): for a layer
 * whose data-gradient kernel takes fp32 while its weight-gradient kernel takes planes */
int viai_bn_act_bwd_p16_twin(const float* dz, const float* y, const float* mean, const float* invstd,
                             const float* scale, const float* shift, float* part, float* sums,
                             float* dgamma, float* dbeta, float* dy, float* dy32, long M, int C, int act, float slope,
                             int training, float* amax, void* stream);
/* (ABI 15) the BatchNorm backward behind a residual join with a ReLU (networks/ResNet.py:46-53): the gradient of the join's output arrives as
 * dz (+ dz2, may be NULL); dres = (dz + dz2) * [zj > 0] is written (M x C floats: the residual branch's gradient) and stands in for dz in
 * viai_bn_act_bwd_p16 with act = none -- the same values as viai_add_act_bwd_from_output + viai_bn_act_bwd_p16, one pass over memory fewer */
int viai_bn_join_bwd_p16(const float* dz, const float* dz2, const float* zj, float* dres, const float* y, const float* mean, const float* invstd,
                         const float* scale, const float* shift, float* part, float* sums, float* dgamma, float* dbeta, float* dy,
                         long M, int C, int training, float* amax, void* stream);
/* x (fp32) = the values a P16 tensor holds, (lead + rem) / S(*amax) */
int viai_p16_decode(const float* p16, float* x, long M, int C, const float* amax, void* stream);
/* viai_conv2d_fwd_amax / viai_conv2d_dgrad_f16 with the gathered tensor pre-split (one source; scale from *x_amax / *dy_amax).
 * On a layer that reports VIAI_P16_OK_FWD_LIN the forward writes stat_part in the linear-tile layout: finalize it with
 * viai_bn_finalize_lin, never with viai_bn_finalize / _tiles (fp32-form launches of the same layer keep viai_conv2d_stat_geom's layout). */
int viai_conv2d_fwd_p16(const viai_conv2d* c, const float* x, const float* wp_fwd, const float* bias, float* y, float* stat_part,
                        int act, const float* x_amax, void* stream);
int viai_conv2d_dgrad_f16_p16(const viai_conv2d* c, const float* dy, const float* wp, float* dx, float* dx2,
                              const float* dy_amax, void* stream);
/* viai_conv2d_wgrad_f16 with pre-split operands (flags: VIAI_P16_DY | VIAI_P16_X); db must be NULL when dy is P16 */
int viai_conv2d_wgrad_f16_p16(const viai_conv2d* c, const float* x, const float* x2, const float* dy,
                              float* ws, float* dw, float* db, int accumulate, const float* dy_amax, const float* x_amax, int flags, void* stream);

/* -------------------------------------------------- launch plans: the train step recorded once, replayed from C
 * Replaces the per-launch host work of `model.optimize_parameters()` (train_whole_sync.py:76).  Protocol:
 *   viai_plan_log_begin();  <stream-capture the step: every library launch notes (kernel, stream)>;  n = viai_plan_log_end();
 *   viai_plan_build(captured hipGraph_t, capture origin stream, &plan);   // reads nodes + edges, never instantiates the graph
 *   viai_plan_replay(plan, stream);                                       // each step: same kernels, arguments, streams, edges
 * The hipGraph_t (it owns the kernel-argument arrays) and every buffer the capture touched must outlive the plan.
 * Kernel, 1-D copy, fill and empty nodes are accepted; anything else returns hipErrorNotSupported.
 * viai_plan_info fills out[0..n) with: nodes, kernels, kernels with a noted stream, copies, fills, streams, events, waits.   */
typedef struct viai_plan viai_plan;
int viai_plan_log_begin(void);
int viai_plan_log_end(void);
int viai_plan_build(void* hip_graph, void* capture_stream, viai_plan** plan);
int viai_plan_replay(viai_plan* plan, void* stream);
int viai_plan_info(const viai_plan* plan, int* out, int n);
void viai_plan_destroy(viai_plan* plan);

#ifdef __cplusplus
}
#endif
#endif /* VIAI_HIP_H */
