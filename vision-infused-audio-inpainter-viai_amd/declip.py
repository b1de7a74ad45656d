"""Clipped peaks restored on the device: bound-constrained Janssen AR restoration (csrc/declip.hip).

    declip_fill        every cluster of listed runs of every row of a batch under its bounds, `sweeps` launches -> (out, filled)
    declip_fill_host   the same rule on numpy arrays, in plain C++ on the host (`viai_declip_host`): no GPU needed
    declip             `find_gaps(clip=...)` + `declip_fill`, the lists never leaving the device -> (out, gaps, filled)
    declip_file        a WAV file in, a WAV file out: only the bytes of the clipped runs change

The rule (include/viai_hip.h states it in full, csrc/viai_declip_rule.h is its arithmetic): a clipped sample keeps its sign and a lower bound
on its magnitude, |x| >= |recorded|.  Clusters are those of `janssen_fill`; a cluster's window reaches `context` beyond its runs and is NOT cut
at neighbouring runs, whose samples it reads as knowns.  Per iteration: Burg fit on the window, Janssen's joint solve of all unknowns, then up
to `rounds` times every estimate inside its bound is pinned at the bound and the rest are solved again; what still violates is clamped.  A
sweep is one launch over all clusters; the next sweep reads the estimates of the one before, so clusters that closed on capacity stop being
walls for each other.  An exact zero of the recording (a dropout) has no bound and is solved freely: one mixed list is one call.

This is an active-set heuristic without release, not an exact quadratic program.  fp64, + - * / only, every sum in a fixed order: the same
bits on the host and on the device, from run to run, and for a row alone or in any batch.  `filled` codes are `janssen_fill`'s (1 solved, 4 no
model, 5 stopped at a pivot, 0 skipped) and come from the last sweep.  There is no fallback for skipped entries.
"""
from __future__ import annotations

import torch

from . import _lib
from .gap_detect import Gaps
from .janssen import _host_lists, _limits

MAX_ROUNDS, MAX_SWEEPS = 8, 16                            # DC_MAX_ROUNDS of csrc/viai_declip_rule.h; sweeps are launches, the cap is this module's

FULL_SCALE = {"u8": 127.0 / 128.0, "s16": 32767.0 / 32768.0, "s24": 8388607.0 / 8388608.0, "s32": 1.0}     # the largest positive sample as decoded


def _extra(what, rounds, sweeps):
    if int(rounds) != rounds or int(sweeps) != sweeps:
        raise ValueError("%s: rounds and sweeps are integers" % what)
    if not (0 <= rounds <= MAX_ROUNDS and 1 <= sweeps <= MAX_SWEEPS):
        raise ValueError("%s: 0 <= rounds <= %d, 1 <= sweeps <= %d" % (what, MAX_ROUNDS, MAX_SWEEPS))
    return int(rounds), int(sweeps)


def declip_fill(wav, gaps, lengths=None, order=32, context=256, iters=2, rounds=3, sweeps=3, max_len=None):
    """wav (B, n) fp32 on the GPU, the clip as recorded; gaps a `Gaps` (or 3-tuple) of int32 count (B,), start (B, K), length (B, K), as
    `find_gaps(clip=...)` leaves them.  Returns (out, filled): out a new tensor with the samples of the solved runs replaced, filled (B, K)
    int32 codes of the last sweep, both on wav's device.

    lengths   (B,) ints: row b holds clamp(lengths[b], 0, n) samples; a run that crosses the end is skipped, a window stops there.
    order, context, max_len   as `janssen_fill`; the window is [first run - context, last run + context) inside the row and is NOT cut at
              other runs.
    iters     fit-solve-pin iterations per sweep (1 .. 16).
    rounds    pin-and-solve-again rounds per iteration (0 .. 8).  0: no bound is used at all (no clamp either); with sweeps=1 that is the
              unconstrained wide-window solve.
    sweeps    launches (1 .. 16), ping-ponging between two clones of wav; the bounds always come from wav.

    The defaults iters=2, rounds=3, sweeps=3 and context=256 are CHOICES taken from a numpy prototype of the rule on a synthetic voiced
    signal, not measurements of this kernel on the device; tools/declip_rate.py measures what the real kernels give.

    `sweeps` launches and one or two clones, no synchronisation.  Gaps that are int32, contiguous and already on wav's device are read where
    they lie.  ValueError for an argument outside its limits, before anything is launched.  ViaiLibraryError for a CPU tensor: no CPU
    fallback (`declip_fill_host` is the host's call)."""
    order, context, iters, max_len = _limits("declip_fill", order, context, iters, max_len)
    rounds, sweeps = _extra("declip_fill", rounds, sweeps)
    if wav.dim() != 2 or wav.size(0) < 1 or wav.size(1) < 1:
        raise ValueError("declip_fill: wav is (B, n)")
    B, n = wav.shape
    if n >= 2 ** 31:
        raise ValueError("declip_fill: %d samples per row; fewer than 2^31" % n)
    count, start, length = (torch.as_tensor(x) for x in tuple(gaps))
    if count.dim() != 1 or count.numel() != B or start.dim() != 2 or start.size(0) != B or start.size(1) < 1 or start.shape != length.shape:
        raise ValueError("declip_fill: gaps are (count (B,), start (B, K), length (B, K)) with B = %d, K >= 1" % B)
    if lengths is not None:
        lengths = torch.as_tensor(lengths).reshape(-1)
        if lengths.numel() != B:
            raise ValueError("declip_fill: lengths holds one entry per row (B = %d)" % B)
    if not wav.is_cuda:
        raise _lib.ViaiLibraryError("declip_fill runs on the GPU only; no CPU fallback (declip_fill_host states the rule on the host)")
    lib = _lib.load()
    from .ops import _stream
    dev = wav.device
    K = start.size(1)
    ref = wav.float().contiguous()                                                                                     # no-ops when already so
    count, start, length = (x.to(device=dev, dtype=torch.int32).contiguous() for x in (count, start, length))
    if lengths is not None:
        lengths = lengths.to(dev).clamp(-1, 0x7fffffff).to(torch.int32).contiguous()
    filled = torch.empty(B, K, dtype=torch.int32, device=dev)
    bufs = (ref.clone(), ref.clone() if sweeps > 1 else None)                # a sweep reads what the last one wrote and writes the other clone
    src = ref
    for s in range(sweeps):
        out = bufs[s & 1]
        _lib.check(lib.viai_declip(ref.data_ptr(), src.data_ptr(), 0 if lengths is None else lengths.data_ptr(), n, B, n, count.data_ptr(),
                                   start.data_ptr(), length.data_ptr(), K, order, context, max_len, iters, rounds, out.data_ptr(), n,
                                   filled.data_ptr(), _stream()), "viai_declip")
        src = out
    return out, filled


def declip_fill_host(wav, gaps, lengths=None, order=32, context=256, iters=2, rounds=3, sweeps=3, max_len=None):
    """`declip_fill` on the host: wav a (B, n) numpy array, gaps three integer arrays.  Returns (out, filled) as numpy arrays, out a contiguous
    fp32 copy of wav with the solved samples replaced.  Needs the built library, not a GPU."""
    import ctypes as C

    import numpy as np
    order, context, iters, max_len = _limits("declip_fill_host", order, context, iters, max_len)
    rounds, sweeps = _extra("declip_fill_host", rounds, sweeps)
    wav = np.asarray(wav, dtype=np.float32)
    if wav.ndim != 2 or wav.shape[0] < 1 or wav.shape[1] < 1:
        raise ValueError("declip_fill_host: wav is (B, n)")
    B, n = wav.shape
    if n >= 2 ** 31:
        raise ValueError("declip_fill_host: %d samples per row; fewer than 2^31" % n)
    ref = np.ascontiguousarray(wav)
    count, start, length, lengths, lp = _host_lists("declip_fill_host", B, gaps, lengths)
    K = start.shape[1]
    filled = np.empty((B, K), dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    lib = _lib.load()
    bufs = (np.array(ref, copy=True), np.array(ref, copy=True) if sweeps > 1 else None)
    src = ref
    for s in range(sweeps):
        out = bufs[s & 1]
        _lib.check(lib.viai_declip_host(p(ref), p(src), lp, n, B, n, p(count), p(start), p(length), K, order, context, max_len, iters, rounds,
                                        p(out), n, p(filled)), "viai_declip_host")
        src = out
    return out, filled


def declip(wav, clip, lengths=None, max_gaps=1024, **fill_kwargs):
    """Find the clipped runs of wav (B, n) on the GPU and restore them: `find_gaps(wav, lengths, threshold=0.0, clip=clip, min_len=1,
    max_gaps=max_gaps)`, then `declip_fill(wav, gaps, lengths, **fill_kwargs)` on the lists where they lie.  Returns (out, gaps, filled).

    clip      |x| >= clip is clipped (clip > 0).
    `find_gaps` cannot switch its silence test off (a negative threshold is refused), so threshold = 0.0 is the least it takes: EXACT ZEROS
    of the recording ARE LISTED too, every one (min_len = 1), and come back as free unknowns -- a zero has no bound.  In audio decoded from
    integer PCM that re-estimates isolated zero crossings from their neighbours; budget max_gaps for them.

    Nothing happens on the host in between and nothing syncs.  A row with more runs than `max_gaps` has its first max_gaps restored and
    says so in gaps.count (count > K): the caller decides, as with `declick` (`declip_file` refuses to write)."""
    if not float(clip) > 0.0:
        raise ValueError("declip: clip > 0 (the level at and beyond which a sample counts as clipped)")
    from .gap_detect import find_gaps
    gaps = find_gaps(wav, lengths, threshold=0.0, clip=clip, min_len=1, max_gaps=max_gaps)
    out, filled = declip_fill(wav, gaps, lengths=lengths, **fill_kwargs)
    return out, gaps, filled


def declip_file(src, dst, clip=None, **kwargs):
    """Declip the WAV file `src` into `dst`; returns (Gaps, WavInfo).  kwargs are `declip`'s.  Channels are rows of one call: read_wav's decode,
    `declip` on the channel planes, `patch_pcm` into the file's own sample bytes, dst = src's header and chunks around the patched data chunk.

    clip      None: the format's full scale for integer PCM, the largest positive sample as decoded (16-bit: 32767 / 32768); a float
              format has no full scale and needs a clip.
    Every byte of dst outside the samples of the listed runs equals src.  SAMPLES RESTORED BEYOND FULL SCALE SATURATE in `patch_pcm`'s
    encode: in an integer dst they come back as full scale, so declipping at clip=None into the same integer format changes little; attenuate
    first, pass a lower clip, or use a float format (f32 / f64 files keep the restored peaks).  A channel with more runs than `max_gaps`
    raises ValueError and nothing is written (count comes to the host once, for this check)."""
    from .wav_io import _data_tensor, decode_pcm, parse_wav, patch_pcm
    with open(src, "rb") as f:
        buf = f.read()
    info = parse_wav(buf)
    if info.frames < 1:
        raise ValueError("declip_file: %s holds no samples" % src)
    if clip is None:
        if info.fmt not in FULL_SCALE:
            raise ValueError("declip_file: %s is %s, a float format has no full scale: pass clip" % (src, info.fmt))
        clip = FULL_SCALE[info.fmt]
    data = _data_tensor(buf, info, "cuda")
    wav = decode_pcm(data, info.fmt, info.channels)
    out, gaps, _ = declip(wav, clip, **kwargs)
    K = gaps.start.size(1)
    over = (gaps.count > K).nonzero().flatten().tolist()
    if over:
        raise ValueError("declip_file: channels %s hold %s runs, the lists hold %d: pass a larger max_gaps"
                         % (over, [int(gaps.count[c]) for c in over], K))
    patched = patch_pcm(data, out, info.fmt, gaps).cpu().numpy().tobytes()
    end = info.data_offset + info.data_bytes
    with open(dst, "wb") as f:
        f.write(buf[:info.data_offset] + patched + buf[end:])
    return gaps, info


class _CallableModule(type(_lib)):
    """`viai_amd.declip` names this module AND its main function: once the module is imported the package attribute is the module, so the
    module itself is callable and hands the call to `declip`.  `viai_amd.declip(wav, clip)` works before and after `import viai_amd.declip`."""

    def __call__(self, *args, **kwargs):
        return declip(*args, **kwargs)


import sys as _sys  # noqa: E402

_sys.modules[__name__].__class__ = _CallableModule
