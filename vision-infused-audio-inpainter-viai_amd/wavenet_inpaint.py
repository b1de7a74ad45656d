"""Filling a masked gap in a waveform with the WaveNet vocoder: the join between the generator, which fills the masked frames of a mel
spectrogram, and `WaveNet.incremental_forward`, which turns a mel into samples.

Only the receptive field R in front of a gap and the gap itself need the sample-by-sample loop.  Per stream b, in samples (hop = the product of
the up-sampling scales, g0 = gap_start * hop, len = gap_len * hop; with gap_unit="samples" g0 = gap_start, len = gap_len):

    window      clip times [w_b, w_b + L),  w_b = g0_b - R,  L = R + max_b len_b          (viai_wn_window_gather)
    forced      window position t is teacher-forced unless R <= t < R + len_b              (the R known samples fill the ring buffers)
    synthesis   ONE incremental_forward call of T = L steps with that mask                 (viai_wavenet_synth_run_forced)
    splice      out = wav outside the gap, the sample of window position R + i - g0_b in it (viai_wn_splice)

Clip times before 0 or at and beyond n read as silence (0.0, class mu // 2, zero conditioning): the start-up state of wavenet.py:305-312.
include/viai_hip.h has the kernels' contracts, DESIGN.md 11.2f the measurement.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib, wavenet as W
from .ops import _ptr, _stream


def _i32(x, dev):
    return torch.as_tensor(x).to(dev).to(torch.int32).reshape(-1).contiguous()


def window_gather(w, length, L, R, wav=None, classes=None, cond=None, silence_class=127):
    """`viai_wn_window_gather`: wav (B, n) floats and / or classes (B, n) integers, cond (B, n, cin) or None; w, length: (B,) window starts and gap
    lengths in samples.  Returns (x (B, L) or None, classes (B, L) int32 or None, cond (B, L, cin) or None, forced (B, L) uint8)."""
    src = wav if wav is not None else classes
    if src is None or src.dim() != 2:
        raise ValueError("window_gather: wav or classes, (B, n)")
    B, n = src.shape
    dev = src.device
    if cond is not None and (cond.dim() != 3 or cond.size(0) != B or cond.size(1) != n or cond.size(2) % 4 != 0 or cond.size(2) < 4):
        raise ValueError("window_gather: cond is (B, n, cin) with cin a multiple of 4 (16-byte rows)")
    w, length = _i32(w, dev), _i32(length, dev)
    if w.numel() != B or length.numel() != B or L < 1 or R < 0:
        raise ValueError("window_gather: w and length hold one entry per stream; L >= 1, R >= 0")
    lib = _lib.load()
    wav = None if wav is None else wav.float().contiguous()
    classes = None if classes is None else classes.to(torch.int32).contiguous()
    cond = None if cond is None else cond.float().contiguous()
    x = None if wav is None else torch.empty(B, L, device=dev)
    k = None if classes is None else torch.empty(B, L, dtype=torch.int32, device=dev)
    co = None if cond is None else torch.empty(B, L, cond.size(2), device=dev)
    forced = torch.empty(B, L, dtype=torch.uint8, device=dev)
    _lib.check(lib.viai_wn_window_gather(_ptr(wav), _ptr(classes), _ptr(cond), w.data_ptr(), length.data_ptr(), _ptr(x), _ptr(k), _ptr(co),
                                         forced.data_ptr(), B, n, int(L), int(R), cond.size(2) if cond is not None else 4, int(silence_class),
                                         _stream()), "viai_wn_window_gather")
    return x, k, co, forced


def splice(wav, gen, g0, length, R, fade=0):
    """`viai_wn_splice`: wav (B, n), gen (B, L) the windows' samples, g0 / length (B,) in samples -> (B, n)."""
    if wav.dim() != 2 or gen.dim() != 2 or gen.size(0) != wav.size(0) or fade < 0:
        raise ValueError("splice: wav (B, n), gen (B, L), fade >= 0")
    B, n = wav.shape
    g0, length = _i32(g0, wav.device), _i32(length, wav.device)
    if g0.numel() != B or length.numel() != B:
        raise ValueError("splice: g0 and length hold one entry per stream")
    wav, gen = wav.float().contiguous(), gen.float().contiguous()
    out = torch.empty_like(wav)
    _lib.check(_lib.load().viai_wn_splice(wav.data_ptr(), gen.data_ptr(), g0.data_ptr(), length.data_ptr(), out.data_ptr(), B, n, gen.size(1), int(R),
                                          int(fade), _stream()), "viai_wn_splice")
    return out


def gaps_from_mask(mask):
    """(B, 1, 1, frames) time mask of `model.make_time_mask` (1 = known, 0 = gap) -> (gap_start, gap_len), (B,) int64 each, in frames.
    A row without a gap gives (0, 0); a row with more than one gap raises ValueError."""
    if mask.dim() != 4 or mask.size(1) != 1 or mask.size(2) != 1:
        raise ValueError("gaps_from_mask: a (B, 1, 1, frames) time mask")
    hole = (mask[:, 0, 0, :] == 0).cpu()
    n = hole.sum(1)
    first = hole.int().argmax(1)
    start = torch.where(n > 0, first, torch.zeros_like(first))
    ar = torch.arange(hole.size(1))[None, :]
    if not bool((hole == ((ar >= start[:, None]) & (ar < (start + n)[:, None]))).all()):
        raise ValueError("gaps_from_mask: a row has more than one gap")
    return start.long(), n.long()


def hop_size(net):
    """samples per conditioning frame: the product of the up-sampling strides (1 without the stack)"""
    hop = 1
    for m in (net.upsample_conv or ()):
        if isinstance(m, nn.ConvTranspose2d):
            hop *= m.stride[1]
    return hop


def _per_stream(x, B, name):
    x = torch.as_tensor(x).detach().cpu().to(torch.int64).reshape(-1)
    if x.numel() == 1:
        x = x.expand(B).clone()
    if x.numel() != B:
        raise ValueError("inpaint_waveform: %s holds one entry per stream (B = %d)" % (name, B))
    return x


def inpaint_waveform(net, wav, c, gap_start, gap_len, uniforms=None, fade=0, return_window=False, gap_unit="frames"):
    """wav (B, n) floats in [-1, 1]; c (B, cin, frames) with n == frames * hop; gap_start / gap_len: frames, per stream ((B,) ints or a tensor, or
    one int for all).  Returns the (B, n) waveform with [gap_start, gap_start + gap_len) regenerated and every other sample copied bit for bit.
    `gap_unit="samples"`: gap_start / gap_len are samples of `wav` (damage does not come in whole frames); the gap must lie inside the n samples.

    One-hot network: the window goes in as mu-law classes (`mulaw_quantize`, mu = out_channels - 1), the call samples (quantize=True) and the classes
    come out through `mulaw_decode`.  Scalar network: raw samples and the mixture-of-logistics sampler.
    `uniforms`: the sampler's draws in WINDOW coordinates, as `incremental_forward` takes them for T = L = receptive_field + the longest gap in
    samples: (B, L) for the one-hot network, (u1 (B, L, 10), u2 (B, L)) for the scalar one.  Window position receptive_field + i is sample i of the gap.
    `fade` > 0 blends the last `fade` samples of each gap linearly from generated to original (viai_wn_splice).
    `return_window=True`: also a dict with the windows' own samples (B, L), their starts (B,) in samples, and the mask of forced steps.
    Stream counts are those of `incremental_forward`'s chain forms (1, 2, 4 or 8)."""
    if gap_unit not in ("frames", "samples"):
        raise ValueError("inpaint_waveform: gap_unit is \"frames\" or \"samples\", not %r" % (gap_unit,))
    if wav.dim() != 2:
        raise ValueError("inpaint_waveform: wav is (B, n)")
    B, n = wav.shape
    hop = hop_size(net)
    if c is None or c.dim() != 3 or c.size(0) != B:
        raise ValueError("inpaint_waveform: c is (B, cin, frames), the conditioning of the whole clip")
    frames = c.size(2)
    if n != frames * hop:
        raise ValueError("inpaint_waveform: %d samples against %d frames of %d samples" % (n, frames, hop))
    if c.size(1) % 4 != 0:
        raise ValueError("inpaint_waveform: the conditioning channel count must be a multiple of 4")
    gs, gl = _per_stream(gap_start, B, "gap_start"), _per_stream(gap_len, B, "gap_len")
    unit, extent = (hop, frames) if gap_unit == "frames" else (1, n)
    if bool((gs < 0).any()) or bool((gl < 0).any()) or bool((gs + gl > extent).any()):
        raise ValueError("inpaint_waveform: a gap must lie inside the clip's %d %s" % (extent, gap_unit))
    if fade < 0:
        raise ValueError("inpaint_waveform: fade >= 0")
    dev = net.first_conv.bias.device
    R = int(net.receptive_field)
    g0, ln = gs * unit, gl * unit
    L = R + int(ln.max())
    w = g0 - R
    wav_d = wav.to(dev).float().contiguous()
    cond = net._upsample(c.to(dev).float()).transpose(1, 2).contiguous()             # (B, n, cin), up-sampled once for the whole clip
    if net.scalar_input:
        x, _, cw, forced = window_gather(w, ln, L, R, wav=wav_d, cond=cond)
        gen = net.incremental_forward(None, c=cw.transpose(1, 2), test_inputs=x.unsqueeze(1), forced=forced, c_upsampled=True,
                                      uniforms=uniforms)[:, 0, :].contiguous()
    else:
        mu = net.out_channels - 1
        cls = W.mulaw_quantize(wav_d, mu)
        _, k, cw, forced = window_gather(w, ln, L, R, classes=cls, cond=cond, silence_class=mu // 2)
        out_cls = net.incremental_forward(None, c=cw.transpose(1, 2), test_inputs=k, forced=forced, c_upsampled=True, uniforms=uniforms,
                                          softmax=True, quantize=True, return_classes=True)
        gen = W.mulaw_decode(out_cls, mu)
    out = splice(wav_d, gen, g0, ln, R, fade)
    if return_window:
        return out, {"samples": gen, "start": w, "forced": forced}
    return out
