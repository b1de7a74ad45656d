"""WaveNet vocoder on the HIP kernels: the reference's `wavenet_vocoder.WaveNet` API and state_dict.

Reference: wavenet_vocoder/wavenet.py:62-393 (WaveNet), modules.py:30-216 (weight-normed Conv1d / Conv1d1x1 /
ConvTranspose2d factories, ResidualConv1dGLU), conv.py:7-65 (incremental Conv1d), mixture.py:25-153 (MoL).
Tensors are (B, 1, T, C) NHWC internally; the module API takes / returns the reference's (B, C, T).
Known latent bugs of the reference that are NOT reproduced as features: `self.softmax(x, dim=1)` TypeError
(wavenet.py:233) and the 5x `self.conv.clear_buffer()` (modules.py:213-216).
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from . import _lib, ops, wavenet_inpaint, wavenet_synth
from .ops import ACT_NONE, ACT_RELU, _c, _ptr, _require, _stream


# ----------------------------------------------------------------------------- autograd ops
class _WeightNorm(torch.autograd.Function):
    """w = g * v / ||v||  per output row (torch.nn.utils.weight_norm, dim=0)."""

    @staticmethod
    def forward(ctx, v, g):
        lib = _lib.load()
        _require(v, g)
        v, g = _c(v), _c(g)
        rows = v.shape[0]
        L = v.numel() // rows
        w = torch.empty_like(v)
        norm = torch.empty(rows, device=v.device, dtype=torch.float32)
        _lib.check(lib.viai_weight_norm_fwd(v.data_ptr(), g.data_ptr(), w.data_ptr(), norm.data_ptr(), rows, L, _stream()), "viai_weight_norm_fwd")
        ctx.save_for_backward(v, g, norm)
        return w

    @staticmethod
    def backward(ctx, dw):
        lib = _lib.load()
        v, g, norm = ctx.saved_tensors
        dw = _c(dw)
        rows = v.shape[0]
        dv, dg = torch.empty_like(v), torch.empty_like(g)
        _lib.check(lib.viai_weight_norm_bwd(dw.data_ptr(), v.data_ptr(), g.data_ptr(), norm.data_ptr(), dv.data_ptr(), dg.data_ptr(),
                                            rows, v.numel() // rows, 0, _stream()), "viai_weight_norm_bwd")
        return dv, dg


def normed_weight(m):
    """effective weight of a (possibly weight-normed) holder module."""
    if hasattr(m, "weight_g"):
        return _WeightNorm.apply(m.weight_v, m.weight_g)
    return m.weight


class _GLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, yc):
        lib = _lib.load()
        _require(y, yc)
        y = _c(y)
        yc = _c(yc) if yc is not None else None
        H = y.shape[-1] // 2
        rows = y.numel() // (2 * H)
        z = torch.empty(y.shape[:-1] + (H,), device=y.device, dtype=torch.float32)
        _lib.check(lib.viai_glu_fwd(y.data_ptr(), _ptr(yc), z.data_ptr(), rows, H, _stream()), "viai_glu_fwd")
        ctx.save_for_backward(y, yc)
        return z

    @staticmethod
    def backward(ctx, dz):
        lib = _lib.load()
        y, yc = ctx.saved_tensors
        dz = _c(dz)
        H = y.shape[-1] // 2
        dy = torch.empty_like(y)
        _lib.check(lib.viai_glu_bwd(dz.data_ptr(), y.data_ptr(), _ptr(yc), dy.data_ptr(), y.numel() // (2 * H), H, _stream()), "viai_glu_bwd")
        return dy, (dy if yc is not None else None)


class _AddScale(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, s):
        lib = _lib.load()
        _require(a, b)
        a = _c(a)
        b = _c(b) if b is not None else None
        out = torch.empty_like(a)
        _lib.check(lib.viai_add_scale(a.data_ptr(), _ptr(b), out.data_ptr(), s, a.numel(), _stream()), "viai_add_scale")
        ctx.s, ctx.hb = s, b is not None
        return out

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        g = _c(g)
        d = torch.empty_like(g)
        _lib.check(lib.viai_add_scale(g.data_ptr(), 0, d.data_ptr(), ctx.s, g.numel(), _stream()), "viai_add_scale")
        return d, (d if ctx.hb else None), None


def add_scale(a, b, s):
    return _AddScale.apply(a, b, float(s))


_U64 = (1 << 64) - 1


def _dropout_launch(x, p, seed, offset, out=None):
    lib = _lib.load()
    _require(x)
    x = _c(x)
    if x.data_ptr() % 16:
        x = x.clone()                                                                 # a view that starts inside a float4: an aligned copy
    y = torch.empty_like(x) if out is None else out
    _lib.check(lib.viai_dropout(x.data_ptr(), y.data_ptr(), x.numel(), p, seed, offset, _stream()), "viai_dropout")
    return y


class _Dropout(torch.autograd.Function):
    """y = x * keep / (1 - p), keep a function of (seed, offset, element index) alone (csrc/dropout.hip): the backward pass runs the same
    kernel on the incoming gradient with the three numbers kept on ctx; no tensor is saved."""

    @staticmethod
    def forward(ctx, x, p, seed, offset):
        ctx.p, ctx.seed, ctx.offset = p, seed, offset
        return _dropout_launch(x, p, seed, offset)

    @staticmethod
    def backward(ctx, g):
        return _dropout_launch(g, ctx.p, ctx.seed, ctx.offset), None, None, None


def _dropout_args(p, seed, offset):
    p = float(p)
    if not 0.0 <= p < 1.0:                                                            # NaN fails both comparisons
        raise ValueError("dropout: p must be in [0, 1), got %r" % (p,))
    return p, int(seed) & _U64, int(offset) & _U64


def dropout(x, p, seed, offset):
    """Training-mode dropout (F.dropout with training=True) with a reproducible mask: element i of the flattened tensor is kept iff word i % 4 of
    Philox4x32-10(counter = (i // 4, offset), key = seed) is >= floor(p * 2^32); kept values are x * float32(1 / (1 - p)), dropped ones +0.
    seed, offset: integers taken modulo 2^64.  p == 0 returns x itself, without a launch."""
    p, seed, offset = _dropout_args(p, seed, offset)
    if p == 0.0:
        return x
    return _Dropout.apply(x, p, seed, offset)


def dropout_mask(shape, p, seed, offset, device="cuda"):
    """the bool keep-mask `dropout` applies to a tensor of this shape with the same (p, seed, offset): the kernel run on ones"""
    p, seed, offset = _dropout_args(p, seed, offset)
    ones = torch.ones(shape, device=device, dtype=torch.float32)
    if p == 0.0:
        return ones.bool()
    return _dropout_launch(ones, p, seed, offset, out=ones) != 0


class _Relu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a):
        lib = _lib.load()
        _require(a)
        a = _c(a)
        out = torch.empty_like(a)
        _lib.check(lib.viai_relu_fwd(a.data_ptr(), out.data_ptr(), a.numel(), _stream()), "viai_relu_fwd")
        ctx.save_for_backward(out)
        return out

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        (out,) = ctx.saved_tensors
        g = _c(g)
        d = torch.empty_like(g)
        _lib.check(lib.viai_relu_bwd(g.data_ptr(), out.data_ptr(), d.data_ptr(), g.numel(), _stream()), "viai_relu_bwd")
        return d


class _Outer(torch.autograd.Function):
    """Conv1d1x1(1, C) on a scalar signal: y[p][c] = x[p]*w[c] + b[c]."""

    @staticmethod
    def forward(ctx, x, w, b):
        lib = _lib.load()
        _require(x, w, b)
        x, w, b = _c(x), _c(w), _c(b)
        Cc = w.numel()
        rows = x.numel()
        y = torch.empty(x.shape[:3] + (Cc,), device=x.device, dtype=torch.float32)
        _lib.check(lib.viai_outer_fwd(x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), rows, Cc, _stream()), "viai_outer_fwd")
        ctx.save_for_backward(x, w)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, w = ctx.saved_tensors
        dy = _c(dy)
        Cc, rows = w.numel(), x.numel()
        part = torch.empty(2 * Cc * lib.viai_outer_bwd_blocks(rows), device=dy.device, dtype=torch.float32)
        dw, db = torch.empty_like(w), torch.empty(Cc, device=dy.device, dtype=torch.float32)
        _lib.check(lib.viai_outer_bwd(dy.data_ptr(), x.data_ptr(), part.data_ptr(), dw.data_ptr(), db.data_ptr(), rows, Cc, 0, _stream()), "viai_outer_bwd")
        return None, dw, db


class _Upsample(torch.autograd.Function):
    """ConvTranspose2d(1,1,(KH,S),stride (1,S),padding ((KH-1)/2,0)) + ReLU on (B,F,T) (wavenet.py:153-164)."""

    @staticmethod
    def forward(ctx, x, w, b):
        lib = _lib.load()
        _require(x, w, b)
        x, w, b = _c(x), _c(w), _c(b)
        B, Fq, T = x.shape
        KH, S = w.shape[2], w.shape[3]
        y = torch.empty((B, Fq, T * S), device=x.device, dtype=torch.float32)
        _lib.check(lib.viai_upsample_fwd(x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), B, Fq, T, KH, S, _stream()), "viai_upsample_fwd")
        ctx.save_for_backward(x, w, y)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, w, y = ctx.saved_tensors
        dy = _c(dy)
        B, Fq, T = x.shape
        KH, S = w.shape[2], w.shape[3]
        part = torch.empty((KH * 16 + 1) * lib.viai_upsample_bwd_blocks(), device=dy.device, dtype=torch.float32)
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dw, db = torch.empty_like(w), torch.empty(1, device=dy.device, dtype=torch.float32)
        _lib.check(lib.viai_upsample_bwd(dy.data_ptr(), y.data_ptr(), x.data_ptr(), w.data_ptr(), part.data_ptr(), _ptr(dx), dw.data_ptr(),
                                         db.data_ptr(), B, Fq, T, KH, S, 0, _stream()), "viai_upsample_bwd")
        return dx, dw, db


def _scale_saved_grad(ctx, g):
    """backward of the two fused losses: the forward pass left d loss / d yhat on ctx, the incoming scalar gradient scales it in place"""
    lib = _lib.load()
    d = ctx.dyh
    g = _c(g)
    _lib.check(lib.viai_scale_by_scalar(d.data_ptr(), g.data_ptr(), d.numel(), _stream()), "viai_scale_by_scalar")
    return d, None, None, None, None


class _MoLLoss(torch.autograd.Function):
    """DiscretizedMixturelogisticLoss: masked mean of the MoL negative log-likelihood (loss_functions.py:43-62)."""

    @staticmethod
    def forward(ctx, yhat, y, mask, num_classes, log_scale_min):
        lib = _lib.load()
        _require(yhat, y, mask)
        yhat, y = _c(yhat), _c(y)
        mask = _c(mask) if mask is not None else None
        pitch = yhat.shape[-1]
        rows = yhat.numel() // pitch
        dev = yhat.device
        loss_rows = torch.empty(rows, device=dev, dtype=torch.float32)
        wrow = torch.empty(rows, device=dev, dtype=torch.float32)
        loss = torch.empty((), device=dev, dtype=torch.float32)
        dyh = torch.empty_like(yhat) if yhat.requires_grad else None
        _lib.check(lib.viai_mol_loss(yhat.data_ptr(), y.data_ptr(), _ptr(mask), loss_rows.data_ptr(), wrow.data_ptr(), loss.data_ptr(),
                                     _ptr(dyh), rows, pitch, 10, float(num_classes), float(log_scale_min), _stream()), "viai_mol_loss")
        ctx.dyh = dyh
        ctx.mark_non_differentiable(loss_rows)
        return loss, loss_rows

    @staticmethod
    def backward(ctx, g, _g2):
        return _scale_saved_grad(ctx, g)


def mol_loss(yhat_nhwc, y, mask=None, num_classes=65536, log_scale_min=math.log(1e-14)):
    """yhat_nhwc: (B,1,T,P>=30) rows [logit|mean|log_scale]x10; y: (B,T[,1]) targets in [-1,1]; mask (B,T[,1])."""
    loss, _ = _MoLLoss.apply(yhat_nhwc, y.reshape(-1), None if mask is None else mask.reshape(-1), num_classes, log_scale_min)
    return loss


def mol_sample(yhat_nhwc, u1, u2, log_scale_min=-7.0):
    """sample_from_discretized_mix_logistic with injected uniforms u1 (rows,10), u2 (rows,)."""
    lib = _lib.load()
    yh = _c(yhat_nhwc)
    pitch = yh.shape[-1]
    rows = yh.numel() // pitch
    out = torch.empty(rows, device=yh.device, dtype=torch.float32)
    _lib.check(lib.viai_mol_sample(yh.data_ptr(), _c(u1).data_ptr(), _c(u2).data_ptr(), out.data_ptr(), rows, pitch, 10,
                                   float(log_scale_min), _stream()), "viai_mol_sample")
    return out


def _require_classes(t):
    if not t.is_cuda:
        raise _lib.ViaiLibraryError("viai ops run on the GPU only (got a %s tensor); no CPU fallback" % t.device)
    if t.dtype != torch.int32:
        raise TypeError("class indices reach the kernels as int32, got %s" % t.dtype)


class _MaskedCE(torch.autograd.Function):
    """MaskedCrossEntropyLoss on NHWC rows: masked mean of the softmax cross-entropy (loss_functions.py:24-40), fused with its gradient."""

    @staticmethod
    def forward(ctx, yhat, target, mask, K, shift):
        lib = _lib.load()
        _require(yhat, mask)
        _require_classes(target)
        yhat, target = _c(yhat), _c(target)
        mask = _c(mask) if mask is not None else None
        B, T = target.shape
        pitch = yhat.shape[-1]
        rows = B * T
        assert yhat.numel() == rows * pitch, (tuple(yhat.shape), tuple(target.shape))
        dev = yhat.device
        loss_rows = torch.empty(rows, device=dev, dtype=torch.float32)
        wrow = torch.empty(2 * rows, device=dev, dtype=torch.float32)
        loss = torch.empty((), device=dev, dtype=torch.float32)
        dyh = torch.empty_like(yhat) if yhat.requires_grad else None
        _lib.check(lib.viai_masked_ce_loss(yhat.data_ptr(), target.data_ptr(), _ptr(mask), loss_rows.data_ptr(), wrow.data_ptr(), loss.data_ptr(),
                                           _ptr(dyh), B, T, K, pitch, shift, _stream()), "viai_masked_ce_loss")
        ctx.dyh = dyh
        ctx.mark_non_differentiable(loss_rows)
        return loss, loss_rows

    @staticmethod
    def backward(ctx, g, _g2):
        return _scale_saved_grad(ctx, g)


def masked_cross_entropy(yhat_nhwc, target, mask=None, shift=0, num_classes=None):
    """yhat_nhwc: (B,1,T,P) logit rows, the first K = num_classes (default P) columns are the classes; target: (B,T[,1]) int32 / int64 classes;
    mask: (B,T[,1]) or (B,T-shift[,1]) floats, entry t weighs logits row t.  shift = s scores row t against target t + s (t < T - s):
    `criterion(y_hat[:, :, :-1], y[:, 1:])` of the reference's training step is shift = 1 on the unsliced tensors."""
    B, T = yhat_nhwc.shape[0], yhat_nhwc.shape[-2]
    K = int(yhat_nhwc.shape[-1] if num_classes is None else num_classes)
    shift = int(shift)
    target = target.reshape(B, T).to(torch.int32)
    if mask is not None:
        mask = mask.reshape(B, -1).float()
        if mask.shape[1] > T - shift:
            mask = mask[:, :T - shift]
        elif mask.shape[1] < T - shift:                                               # sequence_mask without max_len: the missing tail is 0
            mask = torch.nn.functional.pad(mask, (0, T - shift - mask.shape[1]))
        mask = mask.contiguous()
    loss, _ = _MaskedCE.apply(yhat_nhwc, target, mask, K, shift)
    return loss


class _ClassEmbed(torch.autograd.Function):
    """first_conv of the one-hot network on class indices: h[p][:] = w[:, class[p]] + b -- Conv1d1x1(K, C) applied to one-hot rows
    (wavenet.py:118 on the input of data_loader_utils.py:278-281), without the rows."""

    @staticmethod
    def forward(ctx, classes, w, b):
        lib = _lib.load()
        _require(w, b)
        _require_classes(classes)
        classes, w, b = _c(classes), _c(w), _c(b)
        Cc, K = w.shape
        B, T = classes.shape
        wt = torch.empty((K, Cc), device=w.device, dtype=torch.float32)
        h = torch.empty((B, 1, T, Cc), device=w.device, dtype=torch.float32)
        _lib.check(lib.viai_class_embed_fwd(classes.data_ptr(), w.data_ptr(), b.data_ptr(), wt.data_ptr(), h.data_ptr(), B * T, K, Cc, _stream()),
                   "viai_class_embed_fwd")
        ctx.save_for_backward(classes)
        ctx.shape = (Cc, K)
        return h

    @staticmethod
    def backward(ctx, dh):
        lib = _lib.load()
        (classes,) = ctx.saved_tensors
        dh = _c(dh)
        Cc, K = ctx.shape
        rows = classes.numel()
        part = torch.empty(K * Cc * lib.viai_class_embed_bwd_segments(rows), device=dh.device, dtype=torch.float32)
        dw = torch.empty((Cc, K), device=dh.device, dtype=torch.float32)
        db = torch.empty(Cc, device=dh.device, dtype=torch.float32)
        _lib.check(lib.viai_class_embed_bwd(dh.data_ptr(), classes.data_ptr(), part.data_ptr(), dw.data_ptr(), db.data_ptr(), rows, K, Cc, _stream()),
                   "viai_class_embed_bwd")
        return None, dw, db


def receptive_field_size(total_layers, num_cycles, kernel_size, dilation=lambda x: 2 ** x):
    """samples of context one output sees: (k - 1) * sum of the layer dilations + 1 (wavenet_vocoder/wavenet.py:41-59; 505 for the
    reference's 24 layers / 4 cycles / k = 3).  `dilation(i)` maps the position inside a cycle to the dilation."""
    if total_layers % num_cycles != 0:
        raise AssertionError("total_layers must be a multiple of num_cycles")
    per = total_layers // num_cycles
    return (kernel_size - 1) * sum(dilation(i % per) for i in range(total_layers)) + 1


def sequence_mask(sequence_length, max_len=None):
    """(B,) lengths -> (B, max_len) float mask, 1 where t < length (loss_functions.py:11-21); stays on the lengths' device."""
    if max_len is None:
        max_len = int(sequence_length.max())
    t = torch.arange(0, max_len, device=sequence_length.device, dtype=torch.long)
    return (t.unsqueeze(0) < sequence_length.long().unsqueeze(1)).float()


def to_one_hot(tensor, n, fill_with=1.):
    """integer tensor (...) -> float (..., n), one-hot along a new last axis (wavenet_vocoder/mixture.py:108-114)."""
    out = torch.zeros(tuple(tensor.shape) + (n,), dtype=torch.float32, device=tensor.device)
    return out.scatter_(tensor.dim(), tensor.long().unsqueeze(-1), fill_with)


def mulaw_decode(classes, mu=255):
    """mu-law classes (integer tensor, any shape, on the GPU) -> waveform in [-1, 1]: y = 2 k / mu - 1, x = sign(y) ((1 + mu)^|y| - 1) / mu,
    the inverse of the `mulaw_quantize` of the reference's data preparation (utils/librivox.py:66-68; the reference decodes with nnmnkwii's
    `inv_mulaw_quantize`, utils/model_util.py:63-64).  HIP kernel `viai_mulaw_decode`."""
    lib = _lib.load()
    k = classes.to(torch.int32).contiguous()
    out = torch.empty(k.shape, dtype=torch.float32, device=k.device)
    _lib.check(lib.viai_mulaw_decode(k.data_ptr(), out.data_ptr(), k.numel(), int(mu), _stream()), "viai_mulaw_decode")
    return out


def mulaw_quantize(x, mu=255):
    """waveform in [-1, 1] (float tensor, any shape, on the GPU) -> mu-law classes (int64, like the targets the reference's loader builds):
    y = sign(x) log1p(mu |x|) / log1p(mu), class = trunc((y + 1) / 2 * mu) clamped to [0, mu] -- the closed form of the `P.mulaw_quantize`
    of the reference's data preparation (utils/librivox.py:66-74).  HIP kernel `viai_mulaw_quantize`."""
    lib = _lib.load()
    xx = x.to(torch.float32).contiguous()
    out = torch.empty(xx.shape, dtype=torch.int32, device=xx.device)
    _lib.check(lib.viai_mulaw_quantize(xx.data_ptr(), out.data_ptr(), xx.numel(), int(mu), _stream()), "viai_mulaw_quantize")
    return out.long()


def inpaint_waveform(net, wav, c, gap_start, gap_len, uniforms=None, fade=0, return_window=False, gap_unit="frames"):
    """Fill one gap per stream of a waveform with the vocoder `net`: the receptive field in front of every gap is teacher-forced, the gap runs
    free, everything else is copied (viai_amd/wavenet_inpaint.py, documented there).  gap_start / gap_len are frames, or samples with gap_unit="samples"."""
    return wavenet_inpaint.inpaint_waveform(net, wav, c, gap_start, gap_len, uniforms, fade, return_window, gap_unit)


def gaps_from_mask(mask):
    """(B, 1, 1, frames) time mask of `model.make_time_mask` (1 = known, 0 = gap) -> (gap_start, gap_len), two (B,) int64 tensors in frames."""
    return wavenet_inpaint.gaps_from_mask(mask)


# ----------------------------------------------------------------------------- modules
def _wn(m, on):
    return nn.utils.weight_norm(m) if on else m


def Conv1d(in_channels, out_channels, kernel_size=1, padding=0, dilation=1, bias=True, weight_normalization=True,
           dropout=0, std_mul=1.0):
    """modules.py:30-41 (parameter holder; the arithmetic is viai_conv2d_* with kh = 1)."""
    m = nn.Conv1d(in_channels, out_channels, kernel_size, padding=padding, dilation=dilation, bias=bias)
    if weight_normalization:
        std = math.sqrt((std_mul * (1.0 - dropout)) / (m.kernel_size[0] * in_channels))
        m.weight.data.normal_(mean=0, std=std)
        m.bias.data.zero_()
    return _wn(m, weight_normalization)


def Conv1d1x1(in_channels, out_channels, bias=True, weight_normalization=True):
    return Conv1d(in_channels, out_channels, 1, 0, 1, bias, weight_normalization)


def conv1d_apply(x, m, act=ACT_NONE, causal_crop=False):
    """x (B,1,T,Cin) -> (B,1,T',Cout) with holder m (nn.Conv1d, maybe weight-normed)."""
    w = normed_weight(m).unsqueeze(2)                         # (Cout,Cin,1,k)
    k, d, p = m.kernel_size[0], m.dilation[0], m.padding[0]
    return ops.conv_bn_act(x, w, m.bias, None, kernel=(1, k), stride=(1, 1), padding=(0, p), dilation=(1, d),
                           padding2=(-1, 0 if causal_crop else -1), act=act)

class ResidualConv1dGLU(nn.Module):
    """modules.py:84-216."""

    def __init__(self, residual_channels, gate_channels, kernel_size, skip_out_channels=None, cin_channels=-1, gin_channels=-1,
                 dropout=1 - 0.95, padding=None, dilation=1, causal=True, bias=True, weight_normalization=True):
        super().__init__()
        self.dropout = dropout
        # the dropout stream of this layer (plain attributes, not buffers: state_dict() is the reference's): training forward number n
        # uses the mask of (seed, offset = n * 1024 + layer_index)
        self.layer_index, self._drop_seed, self._drop_calls = 0, None, 0
        skip_out_channels = residual_channels if skip_out_channels is None else skip_out_channels
        if padding is None:
            padding = (kernel_size - 1) * dilation if causal else (kernel_size - 1) // 2 * dilation
        self.causal = causal
        self.conv = Conv1d(residual_channels, gate_channels, kernel_size, padding=padding, dilation=dilation, bias=bias,
                           weight_normalization=weight_normalization)
        self.conv1x1c = Conv1d1x1(cin_channels, gate_channels, bias, weight_normalization) if cin_channels > 0 else None
        self.conv1x1g = Conv1d1x1(gin_channels, gate_channels, bias, weight_normalization) if gin_channels > 0 else None
        self.conv1x1_out = Conv1d1x1(gate_channels // 2, residual_channels, bias, weight_normalization)
        self.conv1x1_skip = Conv1d1x1(gate_channels // 2, skip_out_channels, bias, weight_normalization)

    def forward_nhwc(self, x, c=None, g=None):
        residual = x
        if self.training and self.dropout > 0:                                  # modules.py:173-175: the residual keeps the un-dropped input
            assert 0 <= self.layer_index < 1024, "dropout offsets are calls * 1024 + layer_index"
            if self._drop_seed is None:                                         # never seeded: one draw from torch's default CPU generator
                self._drop_seed = int(torch.empty((), dtype=torch.int64).random_())
            x = dropout(x, self.dropout, self._drop_seed, self._drop_calls * 1024 + self.layer_index)
            self._drop_calls += 1
        y = conv1d_apply(x, self.conv, causal_crop=self.causal)                 # (B,1,T,gate)  modules.py:176-181
        yc = None
        if c is not None:
            yc = conv1d_apply(c, self.conv1x1c)                                 # :187-191
        if g is not None:
            yg = conv1d_apply(g, self.conv1x1g)                                 # :194-198
            yc = yg if yc is None else yc + yg
        z = _GLU.apply(y, yc)                                                   # :201
        s = conv1d_apply(z, self.conv1x1_skip)                                  # :204
        out = conv1d_apply(z, self.conv1x1_out)                                 # :207
        return add_scale(out, residual, math.sqrt(0.5)), s                      # :209


class WaveNet(nn.Module):
    """wavenet.py:62-393 (scalar_input=True / mixture-of-logistics output is the reference's configuration)."""

    def __init__(self, out_channels=30, layers=24, stacks=4, residual_channels=512, gate_channels=512, skip_out_channels=256,
                 kernel_size=3, dropout=1 - 0.95, cin_channels=80, gin_channels=-1, n_speakers=None, weight_normalization=True,
                 upsample_conditional_features=True, upsample_scales=(4, 4, 4, 4), freq_axis_kernel_size=3, scalar_input=True,
                 use_speaker_embedding=True):
        super().__init__()
        assert layers % stacks == 0
        self.scalar_input, self.out_channels, self.cin_channels = scalar_input, out_channels, cin_channels
        per = layers // stacks
        self.first_conv = Conv1d1x1(1 if scalar_input else out_channels, residual_channels, True, weight_normalization)
        self.conv_layers = nn.ModuleList([
            ResidualConv1dGLU(residual_channels, gate_channels, kernel_size, skip_out_channels, cin_channels, gin_channels, dropout,
                              dilation=2 ** (i % per), bias=True, weight_normalization=weight_normalization) for i in range(layers)])
        for i, f in enumerate(self.conv_layers):
            f.layer_index = i                                          # the layers of one training forward draw different dropout masks
        self.last_conv_layers = nn.ModuleList([nn.ReLU(inplace=True), Conv1d1x1(skip_out_channels, skip_out_channels, True, weight_normalization),
                                               nn.ReLU(inplace=True), Conv1d1x1(skip_out_channels, out_channels, True, weight_normalization)])
        self.embed_speakers = None
        if gin_channels > 0 and use_speaker_embedding:
            self.embed_speakers = nn.Embedding(n_speakers, gin_channels)
            self.embed_speakers.weight.data.normal_(0, 0.1)
        self.upsample_conv = None
        if upsample_conditional_features:
            self.upsample_conv = nn.ModuleList()
            for s in upsample_scales:
                m = nn.ConvTranspose2d(1, 1, (freq_axis_kernel_size, s), padding=((freq_axis_kernel_size - 1) // 2, 0), dilation=1, stride=(1, s))
                m.weight.data.fill_(1.0 / freq_axis_kernel_size)
                m.bias.data.zero_()
                self.upsample_conv.append(_wn(m, weight_normalization))
                self.upsample_conv.append(nn.ReLU(inplace=True))
        self.receptive_field = receptive_field_size(layers, stacks, kernel_size)

    def seed_dropout(self, seed, calls=0):
        """Fix the dropout masks of training: forward number n (counted from `calls`) of layer l drops by (seed, offset = n * 1024 + l).
        Without it every layer draws its seed from torch's default CPU generator at its first training forward."""
        for f in self.conv_layers:
            f._drop_seed, f._drop_calls = int(seed) & _U64, int(calls)

    def dropout_state(self):
        """{"seed", "calls"}: what load_dropout_state needs to continue the same mask sequence (kept beside a checkpoint; not in state_dict()).
        "seed" is one integer after seed_dropout, None before the first training forward, the per-layer list where the layers drew their own."""
        seeds = [f._drop_seed for f in self.conv_layers]
        return {"seed": seeds[0] if all(v == seeds[0] for v in seeds) else seeds, "calls": [f._drop_calls for f in self.conv_layers]}

    def load_dropout_state(self, d):
        seeds, calls = d["seed"], list(d["calls"])
        if not isinstance(seeds, (list, tuple)):
            seeds = [seeds] * len(self.conv_layers)
        if not len(seeds) == len(calls) == len(self.conv_layers):
            raise ValueError("load_dropout_state: the state is for %d layers, the network has %d" % (len(calls), len(self.conv_layers)))
        for f, sd, n in zip(self.conv_layers, seeds, calls):
            f._drop_seed, f._drop_calls = (None if sd is None else int(sd) & _U64), int(n)

    def has_speaker_embedding(self):
        return self.embed_speakers is not None

    def local_conditioning_enabled(self):
        return self.cin_channels > 0

    def _upsample(self, c):
        """c (B, cin, T') -> (B, cin, T) through the weight-normed transposed-conv stack (wavenet.py:208-215)."""
        if c is None or self.upsample_conv is None:
            return c
        for m in self.upsample_conv:
            if isinstance(m, nn.ReLU):
                continue                                             # fused into the kernel
            c = _Upsample.apply(c, normed_weight(m), m.bias)
        return c

    def _global(self, g, B, T):
        if g is None:
            return None
        if self.embed_speakers is not None:
            g = self.embed_speakers(g.view(B, -1)).transpose(1, 2)
        g = g.unsqueeze(-1) if g.dim() == 2 else g
        return g.expand(B, -1, T).transpose(1, 2).unsqueeze(1).contiguous()          # (B,1,T,gin)

    def forward_nhwc(self, x, c=None, g=None):
        """x (B,1,T), (B,out,T) or, for the one-hot network, integer classes (B,T); returns (B,1,T,P) with P = out_channels padded to a
        multiple of 4."""
        classes = None
        if not self.scalar_input and x.dim() == 2 and not torch.is_floating_point(x):
            classes = x.to(torch.int32)                                               # class form of the first layer: no one-hot tensor
            B, T = classes.shape
        else:
            B, _, T = x.size()
        g_n = self._global(g, B, T)
        c = self._upsample(c)
        c_n = None
        if c is not None:
            assert c.size(-1) == T
            c_n = c.transpose(1, 2).unsqueeze(1).contiguous()                         # (B,1,T,cin)
        if self.scalar_input:
            h = _Outer.apply(x.reshape(B, 1, T).contiguous(), normed_weight(self.first_conv).reshape(-1), self.first_conv.bias)
        elif classes is not None:
            h = _ClassEmbed.apply(classes, normed_weight(self.first_conv).reshape(self.first_conv.out_channels, -1), self.first_conv.bias)
        else:
            h = conv1d_apply(x.transpose(1, 2).unsqueeze(1).contiguous(), self.first_conv)
        skips = None
        for f in self.conv_layers:
            h, s = f.forward_nhwc(h, c_n, g_n)
            skips = s if skips is None else add_scale(skips, s, math.sqrt(0.5))       # wavenet.py:222-226
        h = _Relu.apply(skips)
        h = conv1d_apply(h, self.last_conv_layers[1], act=ACT_RELU)
        last = self.last_conv_layers[3]
        w = normed_weight(last)
        pad = (-self.out_channels) % 4
        bias = last.bias
        if pad:                                                                       # 30 -> 32 output rows (16-byte rows)
            w = torch.cat((w, w.new_zeros((pad,) + tuple(w.shape[1:]))), 0)
            bias = torch.cat((bias, bias.new_zeros(pad)), 0)
        return ops.conv_bn_act(h, w.unsqueeze(2), bias, None, kernel=(1, 1), stride=(1, 1), padding=(0, 0))

    def forward(self, x, c=None, g=None, softmax=False):
        y = self.forward_nhwc(x, c, g)                                                # (B,1,T,P)
        y = y[..., :self.out_channels].squeeze(1).transpose(1, 2)                     # (B, out, T) view
        return torch.softmax(y, dim=1) if softmax else y

    def clear_buffer(self):
        pass                                      # incremental state (ring buffers) is local to incremental_forward

    @torch.no_grad()
    def incremental_forward(self, initial_input=None, c=None, g=None, T=100, test_inputs=None, tqdm=lambda x: x, softmax=True,
                            quantize=True, log_scale_min=-7.0, uniforms=None, use_graph=False, return_logits=False, timing=None,
                            return_classes=False, input_form="auto", forced=None, c_upsampled=False):
        """Sample-by-sample synthesis (wavenet.py:237-364), both configurations of the reference.

        scalar_input=False (one-hot mu-law input, softmax over K = out_channels classes; chain forms only): returns (B, K, T) like the reference --
        softmax / quantize True / True: the one-hot rows of the sampled classes, the class fed back; True / False: the probabilities, fed back as
        they are; False / False: the logits; False / True raises ValueError (the reference hands logits to np.random.choice, which raises).
        `uniforms=` (B, T) draws in [0, 1), one per stream and step, used at every step (teacher-forced ones too, as the reference's
        np.random.choice is); default torch.rand.  Every stream draws its own class (the reference's quantize=True works for B = 1 only).
        `return_classes=True` (with quantize): the (B, T) int64 classes, the (B, K, T) one-hot tensor is never formed.  `test_inputs` /
        `initial_input` in either layout, (B, K, n) or (B, n, K); teacher-forced rows that are exactly one-hot go through the class form of
        the first conv (a row gather), anything else -- or everything, with input_form="dense" -- through the dense form (a K-long product).
        Integer `test_inputs` (B, n) are the classes themselves (class form, no one-hot tensor).

        `forced=` (B, T) bool or uint8 (both networks): which steps are teacher-forced, per stream -- the reference forces a prefix common to
        the batch (wavenet.py:322-327).  The input of step t of stream b is test_inputs[b, t] where forced[b, t], else the previous output
        (at t = 0 the start value); every step still returns the model's own output.  The number of steps is the mask's, `test_inputs` must
        have exactly that length, and what it holds at steps that are not forced is never read.  Chain forms only (the pipelined form is not
        taken).  `c_upsampled=True`: `c` is already at the sample rate, (B, cin, T), and the up-sampling stack is skipped.

        scalar_input=True (mixture of logistics):

        A time step = first conv, 2 GEMV-batch kernels per layer, head + MoL sample.  Default: `viai_wavenet_synth_run` loops over the
        steps in C with the time index passed by value; `use_graph=True`: `viai_wavenet_synth_step` (time index on the device, the first
        conv advances it) captured once into a HIP graph and replayed.
        `uniforms=(u1 (B,T,10), u2 (B,T))` injects the sampler's two uniform draws (parity tests); default torch.rand.
        `timing={"warmup": W}` (bench.py): the first W time steps run untimed, the remaining T - W are bracketed by device
        synchronisations and reported as timing["ms"] / timing["steps"] (set-up -- weight norm, linearised weights -- excluded)."""
        return wavenet_synth.incremental_forward(self, initial_input, c, g, T, test_inputs, tqdm, softmax, quantize, log_scale_min, uniforms, use_graph,
                                                 return_logits, timing, return_classes, input_form, forced, c_upsampled)

    def make_generation_fast_(self):
        def rm(m):
            try:
                nn.utils.remove_weight_norm(m)
            except ValueError:
                return
        self.apply(rm)


class DiscretizedMixturelogisticLoss(nn.Module):
    """loss_functions.py:43-62; input (B, C, T) or the NHWC tensor of WaveNet.forward_nhwc, target (B, T, 1)."""

    def __init__(self, quantize_channels=65536, log_scale_min=math.log(1e-14)):
        super().__init__()
        self.quantize_channels, self.log_scale_min = quantize_channels, log_scale_min

    def forward(self, input, target, lengths=None, mask=None, max_len=None):
        if lengths is None and mask is None:
            raise RuntimeError("Should provide either lengths or mask")
        if mask is None:
            mask = sequence_mask(lengths, max_len).unsqueeze(-1)
        if input.dim() == 3:                                                          # (B, C, T) -> NHWC rows, padded to 32
            B, Cc, T = input.shape
            yh = torch.nn.functional.pad(input.transpose(1, 2), (0, (-Cc) % 4)).reshape(B, 1, T, -1).contiguous()
        else:
            yh = input
        return mol_loss(yh, target, mask, self.quantize_channels, self.log_scale_min)


class MaskedCrossEntropyLoss(nn.Module):
    """loss_functions.py:24-40.  input: (B, K, T), (B, K, T, 1) (what the reference's criterion receives, train.py's __train_step) or the NHWC
    tensor (B, 1, T, P) of WaveNet.forward_nhwc (its first `num_classes` columns, all P by default); target (B, T, 1) or (B, T), int32 or int64.
    `shift = s` scores input step t against target step t + s: criterion(y_hat, y, lengths=..., max_len=T - 1, shift=1) is the reference's
    criterion(y_hat[:, :, :-1], y[:, 1:], lengths=..., max_len=T - 1) without the sliced copies."""

    def __init__(self, num_classes=None):
        super().__init__()
        self.num_classes = num_classes

    def forward(self, input, target, lengths=None, mask=None, max_len=None, shift=0):
        if lengths is None and mask is None:
            raise RuntimeError("Should provide either lengths or mask")
        if mask is None:
            mask = sequence_mask(lengths, max_len).unsqueeze(-1)
        K = self.num_classes
        if input.dim() == 4 and input.size(1) == 1:                                   # NHWC rows
            yh = input
        else:                                                                         # (B, K, T[, 1]) -> NHWC rows, padded to whole float4s
            if input.dim() == 4:
                input = input.squeeze(-1)
            B, Kc, T = input.shape
            K = Kc if K is None else K
            yh = torch.nn.functional.pad(input.transpose(1, 2), (0, (-Kc) % 4)).reshape(B, 1, T, -1).contiguous()
        return masked_cross_entropy(yh, target, mask.to(yh.device), shift, K)
