"""Clips at any sample rate: a rational-ratio polyphase resampler on the device (csrc/wav_resample.hip).

    Resampler         sr_in -> sr_out, Kaiser-windowed sinc, one launch per batch; a window of outputs can be written into an existing tensor
    gap_at_rate       the outputs whose filter support meets a gap of the input: the resampler's counterpart of `gap_frames`
    inpaint_at_rate   `AudioInpainter` on a clip at its own rate: down, widen the gap, inpaint, up, only the gap written back

Output k sits at input time k M / L (L = sr_out / gcd, M = sr_in / gcd) and is the dot product of 2 H + 1 input samples around it with the row of
the tap table that belongs to the phase (k M) mod L.  The taps are computed on the host in fp64 and rounded once; the kernel accumulates each output
in fp32 in tap order, so a row gives the same bits alone, in a batch and under a window.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from .ops import _stream


def _per_row(x, B, what):
    """(B,) int64 on the host from one int, a sequence or a tensor"""
    x = torch.as_tensor(x).detach().cpu().to(torch.int64).reshape(-1)
    if x.numel() == 1:
        x = x.expand(B).clone()
    if x.numel() != B:
        raise ValueError("%s holds one entry per stream (B = %d)" % (what, B))
    return x


def _plan(sr_in, sr_out, zeros):
    L, M, H, T = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    err = _lib.load().viai_wav_resample_geom(int(sr_in), int(sr_out), int(zeros), C.byref(L), C.byref(M), C.byref(H), C.byref(T))
    if err != 0:
        raise ValueError("Resampler: no plan for %r Hz -> %r Hz with %r zero crossings (rates and zeros >= 1, a table of at most 4 Mi taps)"
                         % (sr_in, sr_out, zeros))
    return L.value, M.value, H.value, T.value


class Resampler:
    """sr_in -> sr_out.  zeros: zero crossings of the sinc on each side at the lower of the two rates; rolloff: the cut-off as a share of the lower
    Nyquist frequency; beta: the Kaiser window's.  The plan is built once.  With `device` the taps are uploaded there at once and a call on another
    device is refused; without it they follow the first call's device (and are uploaded again when a later call is on another one).
    `.L`, `.M`, `.H`, `.T`: the ratio L / M in lowest terms, the filter's half-width in input samples and its taps (2 H + 1)."""

    def __init__(self, sr_in, sr_out, zeros=24, rolloff=0.945, beta=8.6, device=None):
        if int(sr_in) != sr_in or int(sr_out) != sr_out or int(zeros) != zeros:
            raise ValueError("Resampler: sample rates and zeros are integers")
        if int(sr_in) == int(sr_out):
            raise ValueError("Resampler: %d Hz to %d Hz is no resampling" % (sr_in, sr_out))
        if not 0.0 < float(rolloff) <= 1.0 or not 0.0 <= float(beta) < 700.0:
            raise ValueError("Resampler: 0 < rolloff <= 1 and 0 <= beta < 700")
        self.sr_in, self.sr_out, self.zeros, self.rolloff, self.beta = int(sr_in), int(sr_out), int(zeros), float(rolloff), float(beta)
        self.L, self.M, self.H, self.T = _plan(sr_in, sr_out, zeros)
        self._taps = self._first = None
        self.device = None
        if device is not None:
            self.device = self._table(torch.device(device))[0].device      # as torch names it, index included

    def host_table(self):
        """(taps, first): the (T, L) float32 table (tap-major, period order: row q of a period is column q) and the (L,) int32 offsets
        floor(q M / L), on the host (`viai_wav_resample_taps`)"""
        taps = torch.empty(self.T, self.L, dtype=torch.float32)
        first = torch.empty(self.L, dtype=torch.int32)
        _lib.check(_lib.load().viai_wav_resample_taps(self.sr_in, self.sr_out, self.zeros, self.rolloff, self.beta, taps.data_ptr(), first.data_ptr()),
                   "viai_wav_resample_taps")
        return taps, first

    def _table(self, dev):
        if self._taps is None or self._taps.device != dev:
            taps, first = self.host_table()
            self._taps, self._first = taps.to(dev), first.to(dev)
        return self._taps, self._first

    def out_len(self, n):
        """ceil(n L / M): the outputs of n input samples"""
        return int(_lib.load().viai_wav_resample_out_len(int(n), self.L, self.M))

    def launch_form(self):
        """(pp, lt, g, span): the launch form a call takes (`viai_wav_resample_form`, host arithmetic).  A tile is lt * g * pp consecutive
        outputs and stages span words of LDS.  pp = 4: the period form (lt = L, four outputs per work item, g periods per pass); pp = 1: the
        consecutive form (one output per item, lt of 1024 .. 64); pp = 0: no tile fits 64 KiB of LDS and a call is refused."""
        v = [C.c_int() for _ in range(4)]
        _lib.check(_lib.load().viai_wav_resample_form(self.L, self.M, self.H, *[C.byref(x) for x in v]), "viai_wav_resample_form")
        return tuple(x.value for x in v)

    def __call__(self, wav, lengths=None, out=None, window=None, out_len=None):
        """wav (B, n) floats on the GPU -> (B, m), m = ceil(n L / M), or (B, out_len).

        lengths   (B,) ints: row b holds lengths[b] samples, the rest of it reads as zero.
        out_len   the number of outputs per row instead of m.  Outputs past m follow the same formula on the zero-extended clip; they are exact
                  zeros from ceil((n + H) L / M) on, so asking for more pads the result in the same pass.
        window    (start, end), ints or one per row: only the outputs in [start, end) are computed and written.
        out       (B, >= m) float32 on the GPU with contiguous rows, written in place and returned; every element outside the window keeps its
                  bits.  Without `out` a windowed call returns zeros there."""
        if wav.dim() != 2 or wav.size(0) < 1 or wav.size(1) < 1:
            raise ValueError("Resampler: wav is (B, n)")
        B, n = wav.shape
        m = self.out_len(n) if out_len is None else int(out_len)
        if m < 1 or m > 0x7fffffff:
            raise ValueError("Resampler: %d outputs per row; 1 to 2^31 - 1" % m)
        if out is not None:
            if out.dim() != 2 or out.size(0) != B or out.size(1) < m or out.dtype != torch.float32 or out.stride(1) != 1:
                raise ValueError("Resampler: out is (B, >= %d) float32 with contiguous rows, not %s %s" % (m, tuple(out.shape), out.dtype))
        if lengths is not None:
            lengths = _per_row(lengths, B, "Resampler: lengths") if not (torch.is_tensor(lengths) and lengths.is_cuda) else lengths.reshape(-1)
            if lengths.numel() != B:
                raise ValueError("Resampler: lengths holds one entry per stream (B = %d)" % B)
            if not lengths.is_cuda and (bool((lengths < 0).any()) or bool((lengths > n).any())):
                raise ValueError("Resampler: a row's length lies in [0, %d]" % n)
        if window is not None:
            if len(window) != 2:
                raise ValueError("Resampler: window is (start, end)")
            w0, w1 = _per_row(window[0], B, "Resampler: window start"), _per_row(window[1], B, "Resampler: window end")
        if not wav.is_cuda or (out is not None and not out.is_cuda):
            raise _lib.ViaiLibraryError("Resampler runs on the GPU only; no CPU fallback")
        if self.device is not None and wav.device != self.device:
            raise ValueError("Resampler: built for %s, called with a clip on %s" % (self.device, wav.device))
        wav = wav.float()
        if wav.stride(1) != 1 or (B > 1 and wav.stride(0) < n):             # transposed, expanded or overlapping rows: a copy with plain rows
            wav = wav.contiguous()
        dev = wav.device
        taps, first = self._table(dev)
        if out is None:
            out = torch.empty(B, m, device=dev) if window is None else torch.zeros(B, m, device=dev)
        o0 = o1 = 0
        if window is not None:
            lim = 0x7fffffff
            bounds = torch.stack((w0.clamp(-lim, lim), w1.clamp(-lim, lim))).to(torch.int32).to(dev)          # one upload for both vectors
            o0, o1 = bounds[0].data_ptr(), bounds[1].data_ptr()
        x_stride = wav.stride(0) if B > 1 else n
        y_stride = out.stride(0) if B > 1 else out.size(1)
        if y_stride < m:
            raise ValueError("Resampler: the rows of out overlap")
        if lengths is not None:
            lengths = lengths.to(dev).clamp(0, n).to(torch.int32).contiguous()     # the kernel clamps to the row stride only
        elif x_stride != n:
            lengths = torch.full((B,), n, dtype=torch.int32, device=dev)           # a view of wider rows: what lies behind n is not the clip
        _lib.check(_lib.load().viai_wav_resample(wav.data_ptr(), 0 if lengths is None else lengths.data_ptr(), taps.data_ptr(), first.data_ptr(),
                                                 out.data_ptr(), o0, o1, B, x_stride, y_stride, m, self.L, self.M, self.H, self.T, _stream()),
                   "viai_wav_resample")
        return out if out.size(1) == m else out[:, :m]


def gap_at_rate(gap_start, gap_len, resampler, m):
    """The outputs of `resampler` that a gap of its input reaches.  The gap [gap_start, gap_start + gap_len) is in samples of the input; output k
    reads the inputs [i0 - H, i0 + H], i0 = floor(k M / L), and is reached when the two meet.  Returns (start, len) on the output grid, clipped to
    [0, m); an empty gap gives (0, 0).  Two ints for int arguments; two lists, one entry per stream, for sequences or tensors
    (`viai_gap_at_rate`; pure host arithmetic)."""
    gs = torch.as_tensor(gap_start).detach().cpu().to(torch.int64).reshape(-1)
    gl = torch.as_tensor(gap_len).detach().cpu().to(torch.int64).reshape(-1)
    if gs.numel() == 1 and gl.numel() > 1:
        gs = gs.expand(gl.numel())
    if gl.numel() == 1 and gs.numel() > 1:
        gl = gl.expand(gs.numel())
    if gs.numel() != gl.numel():
        raise ValueError("gap_at_rate: gap_start and gap_len hold one entry per stream")
    if int(m) < 0:
        raise ValueError("gap_at_rate: m >= 0")
    fn = _lib.load().viai_gap_at_rate
    start, length = [], []
    k0, k1 = C.c_long(), C.c_long()
    for g0, n in zip(gs.tolist(), gl.tolist()):
        if fn(g0, g0 + max(n, 0), resampler.L, resampler.M, resampler.H, int(m), C.byref(k0), C.byref(k1)) != 0:
            raise ValueError("gap_at_rate: a gap of %d samples at %d is out of range" % (n, g0))
        start.append(k0.value)
        length.append(k1.value - k0.value)
    if isinstance(gap_start, int) and isinstance(gap_len, int):
        return start[0], length[0]
    return start, length


_PLANS = {}


def _resampler(sr_in, sr_out):
    key = (int(sr_in), int(sr_out))
    if key not in _PLANS:
        _PLANS[key] = Resampler(sr_in, sr_out)
    return _PLANS[key]


def inpaint_at_rate(inpainter, wav, sample_rate, gap_start, gap_len, uniforms=None, fade=0, video=None, flow=None, return_parts=False):
    """`inpainter(wav, gap_start, gap_len)` for a clip at `sample_rate` instead of the front end's.  wav (B, n) on the GPU, gaps in samples of wav,
    one int or one per stream, length 0 = no gap.

        down     wav -> the front end's rate, zero-padded to the next whole number of hops in the same pass
        widen    the gap on that grid is every sample whose filter support meets the gap (`gap_at_rate`): the samples of the gap reach no
                 sample outside it, so the gap is not silenced at the source rate
        inpaint  `inpainter(low, start, len, ...)` unchanged; its own checks (1, 2, 4 or 8 streams, the width rule) apply
        up       back to `sample_rate`, only the outputs of [gap_start, gap_start + gap_len), written into a clone of wav

    The result equals wav bit for bit outside the gaps.  `sample_rate` equal to the front end's calls the inpainter directly.
    `return_parts=True`: also a dict with `low` (the clip at the front end's rate), `low_gap` (start, len per stream), `low_out` (the inpainter's
    result) and the inpainter's own parts."""
    cfg = inpainter.front.cfg
    rate, hop = int(cfg.sample_rate), int(cfg.hop_size)
    if int(sample_rate) != sample_rate or sample_rate < 1:
        raise ValueError("inpaint_at_rate: sample_rate is a positive integer")
    if int(sample_rate) == rate:
        return inpainter(wav, gap_start, gap_len, video=video, flow=flow, uniforms=uniforms, fade=fade, return_parts=return_parts)
    if wav.dim() != 2 or wav.size(0) < 1 or wav.size(1) < 1:
        raise ValueError("inpaint_at_rate: wav is (B, n)")
    B, n = wav.shape
    gs, gl = _per_row(gap_start, B, "inpaint_at_rate: gap_start"), _per_row(gap_len, B, "inpaint_at_rate: gap_len")
    if bool((gs < 0).any()) or bool((gl < 0).any()) or bool((gs + gl > n).any()):
        raise ValueError("inpaint_at_rate: a gap must lie inside the clip's %d samples" % n)
    if not wav.is_cuda:
        raise _lib.ViaiLibraryError("inpaint_at_rate runs on the GPU only; no CPU fallback")
    down, up = _resampler(sample_rate, rate), _resampler(rate, sample_rate)
    m = -(-down.out_len(n) // hop) * hop
    low = down(wav, out_len=m)
    start, length = gap_at_rate(gs, gl, down, m)
    got = inpainter(low, start, length, video=video, flow=flow, uniforms=uniforms, fade=fade, return_parts=return_parts)
    low_out, parts = got if return_parts else (got, None)
    out = wav.float().clone(memory_format=torch.contiguous_format)
    up(low_out, out=out, window=(gs, gs + gl), out_len=n)
    if return_parts:
        parts = dict(parts)
        parts.update(low=low, low_gap=(start, length), low_out=low_out)
        return out, parts
    return out
