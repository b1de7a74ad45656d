"""Where a waveform holds clicks, found on the device (csrc/click_detect.hip), and `declick`: detect, then interpolate.

    find_clicks        impulsive damage (clicks, crackle, bit errors, a single wild sample) of every row of a batch -> Gaps(count, start, length)
    find_clicks_host   the same rule on a numpy array, in plain C++ on the host (`viai_click_detect_host`): no GPU needed
    declick            `find_clicks` + `ar_fill` (or `janssen_fill`, method="janssen"), the lists never leaving the device -> (out, gaps, filled)
    declick_host       `find_clicks_host` + `ar_fill_host` (or `janssen_fill_host`)
    declick_file       a WAV file in, a WAV file out: only the bytes of the detected runs change

The rule (include/viai_hip.h states it in full, csrc/viai_click_rule.h is its arithmetic): every tile of 4096 samples gets an all-pole model by
Burg's method (the fit of `ar_fill`), the signal is run through the prediction-error filter, and a sample is flagged when its squared residual
exceeds k^2 times the tile's robust variance (the mean of the squared residuals, re-taken `passes` times over the samples under the cut) or
floor^2, whichever is larger; a non-finite sample is always flagged.  Flags are widened by `guard` samples on both sides and then go through
the run rule of `find_gaps` (min_len, merge_within, max_gaps).  The lists are exact integers: the same on the host and on the device, from run to
run, and for a row alone or in any batch.

A click is neither silent nor clipped, so `find_gaps` does not see it, and a dropout is no outlier of a residual, so `find_clicks` does not see
that.  Merging click runs with dropout runs into one list is OUT OF SCOPE here: run `declick` on the clip first and `repair` on its result.
"""
from __future__ import annotations

import torch

from . import _lib
from .gap_detect import Gaps

MAX_ORDER, MAX_PASSES, MAX_GUARD = 128, 4, 64             # AR_MAX_ORDER, CD_MAX_PASSES, CD_MAX_GUARD of csrc/viai_click_rule.h


def _rule(what, order, k, passes, guard, floor, min_len, merge_within, max_gaps):
    ints = (order, passes, guard, min_len, merge_within, max_gaps)
    if any(int(v) != v for v in ints):
        raise ValueError("%s: order, passes, guard, min_len, merge_within and max_gaps are integers" % what)
    if not (1 <= order <= MAX_ORDER and 0 <= passes <= MAX_PASSES and 0 <= guard <= MAX_GUARD):
        raise ValueError("%s: 1 <= order <= %d, 0 <= passes <= %d, 0 <= guard <= %d" % (what, MAX_ORDER, MAX_PASSES, MAX_GUARD))
    if min_len < 1 or merge_within < 0 or max_gaps < 1 or max(min_len, merge_within, max_gaps) > 0x7fffffff:
        raise ValueError("%s: min_len >= 1, merge_within >= 0, max_gaps >= 1" % what)
    if not 0.0 < float(k) <= 3.4028234663852886e38:
        raise ValueError("%s: k > 0 and finite" % what)
    if not float(floor) >= 0.0:
        raise ValueError("%s: floor >= 0 (an amplitude; 0: no floor)" % what)
    return (int(order), float(k), int(passes), int(guard), float(floor), int(min_len), int(merge_within), int(max_gaps))


def find_clicks(wav, lengths=None, order=32, k=5.0, passes=2, guard=2, floor=0.0, min_len=1, merge_within=8, max_gaps=64):
    """wav (B, n) fp32 on the GPU -> Gaps(count, start, length), int32 tensors on wav's device, K = max_gaps: what `ar_fill` and `patch_pcm` read.

    lengths       (B,) ints, a tensor on either side or a sequence: row b holds clamp(lengths[b], 0, n) samples; nothing behind is read or listed.
    order         the model order; a tile of C samples uses min(order, C // 2).  The first `order` samples of a row are never judged.
    k             a sample is a click when |residual| > k times the tile's robust scale.  The default 5 is a CHOICE: large enough that a
                  Gaussian residual gives no flag in minutes of signal, small enough for clicks a listener hears.
    passes        how often the scale is re-taken over the samples under the cut (0 .. 4); 0 is the plain mean, which a loud click drags up.
    guard         samples added to both sides of every flag (0 .. 64): the residual sees a click's onset, the damage rings on for a few samples.
    floor         an amplitude: residuals below it are never clicks (digital silence has a scale of 0 and would flag dither otherwise).
    min_len, merge_within, max_gaps   the run rule of `find_gaps`; count is the true number and may exceed max_gaps.

    Four launches for the batch, no synchronisation, and no copy to the host.  The workspace (2 bits per sample and 52 bytes per 4096-sample
    tile) is allocated per call from torch's caching allocator.  A wav that is not fp32 or whose rows are not contiguous is converted first (a
    copy).  ViaiLibraryError for a CPU tensor: no CPU fallback (`find_clicks_host` is the host's call)."""
    order, k, passes, guard, floor, min_len, merge_within, K = _rule("find_clicks", order, k, passes, guard, floor, min_len, merge_within, max_gaps)
    if wav.dim() != 2 or wav.size(0) < 1 or wav.size(1) < 1:
        raise ValueError("find_clicks: wav is (B, n)")
    B, n = wav.shape
    if n >= 2 ** 31:
        raise ValueError("find_clicks: %d samples per row; fewer than 2^31" % n)
    if lengths is not None:
        lengths = torch.as_tensor(lengths).reshape(-1)
        if lengths.numel() != B:
            raise ValueError("find_clicks: lengths holds one entry per row (B = %d)" % B)
    if not wav.is_cuda:
        raise _lib.ViaiLibraryError("find_clicks runs on the GPU only; no CPU fallback (find_clicks_host states the rule on the host)")
    lib = _lib.load()
    from .ops import _stream
    wav = wav.float()
    if wav.stride(1) != 1 or (B > 1 and wav.stride(0) < n):
        wav = wav.contiguous()
    dev = wav.device
    stride = wav.stride(0) if B > 1 else n
    if lengths is not None:
        lengths = lengths.to(dev).clamp(-1, 0x7fffffff).to(torch.int32).contiguous()
    nbytes = int(lib.viai_click_detect_ws_bytes(B, n, K))
    if nbytes < 1:
        raise ValueError("find_clicks: no launch geometry for B = %d, n = %d" % (B, n))
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
    count = torch.empty(B, dtype=torch.int32, device=dev)
    start = torch.empty(B, K, dtype=torch.int32, device=dev)
    length = torch.empty(B, K, dtype=torch.int32, device=dev)
    _lib.check(lib.viai_click_detect(wav.data_ptr(), 0 if lengths is None else lengths.data_ptr(), stride, B, n, order, k, passes, guard, floor,
                                     min_len, merge_within, K, count.data_ptr(), start.data_ptr(), length.data_ptr(), ws.data_ptr(), _stream()),
               "viai_click_detect")
    return Gaps(count, start, length)


def find_clicks_host(wav, lengths=None, order=32, k=5.0, passes=2, guard=2, floor=0.0, min_len=1, merge_within=8, max_gaps=64):
    """`find_clicks` on the host: wav a (B, n) numpy array (a view of wider rows is read in place), the rule in plain C++ loops from the same
    headers (`viai_click_detect_host`).  Returns Gaps of int32 numpy arrays.  Needs the built library, not a GPU."""
    import ctypes as C

    import numpy as np
    order, k, passes, guard, floor, min_len, merge_within, K = _rule("find_clicks_host", order, k, passes, guard, floor, min_len, merge_within,
                                                                     max_gaps)
    wav = np.asarray(wav, dtype=np.float32)
    if wav.ndim != 2 or wav.shape[0] < 1 or wav.shape[1] < 1:
        raise ValueError("find_clicks_host: wav is (B, n)")
    B, n = wav.shape
    if wav.strides[1] != 4 or (B > 1 and (wav.strides[0] % 4 != 0 or wav.strides[0] < 4 * n)):
        wav = np.ascontiguousarray(wav)
    stride = wav.strides[0] // 4 if B > 1 else n           # one row: numpy may report any stride for it
    if n >= 2 ** 31:
        raise ValueError("find_clicks_host: %d samples per row; fewer than 2^31" % n)
    lp = None
    if lengths is not None:
        lengths = np.ascontiguousarray(np.clip(np.asarray(lengths, dtype=np.int64).reshape(-1), -1, 0x7fffffff), dtype=np.int32)
        if lengths.size != B:
            raise ValueError("find_clicks_host: lengths holds one entry per row (B = %d)" % B)
        lp = lengths.ctypes.data_as(C.c_void_p)
    count = np.empty(B, dtype=np.int32)
    start = np.empty((B, K), dtype=np.int32)
    length = np.empty((B, K), dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    _lib.check(_lib.load().viai_click_detect_host(p(wav), lp, stride, B, n, order, k, passes, guard, floor, min_len, merge_within, K, p(count),
                                                  p(start), p(length)), "viai_click_detect_host")
    return Gaps(count, start, length)


def _method(what, method, ar_iters):
    if method not in ("burg", "janssen"):
        raise ValueError("%s: method is 'burg' or 'janssen'" % what)
    if method == "burg" and ar_iters is not None:
        raise ValueError("%s: ar_iters belongs to method='janssen'" % what)
    return {} if ar_iters is None else {"iters": ar_iters}


def declick(wav, lengths=None, ar_order=32, ar_context=1024, method="burg", ar_iters=None, **find_clicks_kwargs):
    """Find the clicks of wav (B, n) on the GPU and interpolate them: `find_clicks(wav, lengths, **find_clicks_kwargs)`, then
    `ar_fill(wav, gaps, lengths, order=ar_order, context=ar_context)` on the lists where they lie.  Returns (out, gaps, filled).

    method   "burg" (the default): `ar_fill`, every run on its own.  "janssen": `janssen_fill(..., iters=ar_iters)` (default 3), runs that
             lie within ar_context of each other solved jointly, which is what dense crackle needs; ar_context is then at most 1024, runs
             longer than the rule allows come back with filled = 0 and are NOT handed to `ar_fill`.

    Nothing happens on the host in between: five launches and a clone, no synchronisation.  out is a new tensor; every sample outside the
    listed runs, and every row without a click, keeps its bits.  A row with more runs than `max_gaps` has its first max_gaps filled and says
    so in gaps.count: the caller decides (`declick_file` refuses to write)."""
    extra = _method("declick", method, ar_iters)
    gaps = find_clicks(wav, lengths, **find_clicks_kwargs)
    if method == "janssen":
        from .janssen import janssen_fill
        out, filled = janssen_fill(wav, gaps, lengths=lengths, order=ar_order, context=ar_context, **extra)
    else:
        from .ar_fill import ar_fill
        out, filled = ar_fill(wav, gaps, lengths=lengths, order=ar_order, context=ar_context)
    return out, gaps, filled


def declick_host(wav, lengths=None, ar_order=32, ar_context=1024, method="burg", ar_iters=None, **find_clicks_kwargs):
    """`declick` on numpy arrays: `find_clicks_host` + `ar_fill_host` (or `janssen_fill_host`).  Needs the built library, not a GPU."""
    import numpy as np

    extra = _method("declick_host", method, ar_iters)
    wav = np.array(np.asarray(wav, dtype=np.float32), order="C", copy=True)      # rows with their own strides, whatever view came in
    gaps = find_clicks_host(wav, lengths, **find_clicks_kwargs)
    if method == "janssen":
        from .janssen import janssen_fill_host
        out, filled = janssen_fill_host(wav, gaps, lengths=lengths, order=ar_order, context=ar_context, **extra)
    else:
        from .ar_fill import ar_fill_host
        out, filled = ar_fill_host(wav, gaps, lengths=lengths, order=ar_order, context=ar_context)
    return out, gaps, filled


def declick_file(src, dst, **kwargs):
    """Declick the WAV file `src` into `dst`; returns (Gaps, WavInfo).  kwargs are `declick`'s (method="janssen" and ar_iters among them).
    Channels are rows of one call:

        1  read_wav(src, mono=False): the data chunk goes to the device once
        2  declick on the channel planes
        3  patch_pcm into the file's own sample bytes: only the samples of the listed runs are re-encoded
        4  dst = src's header and chunks around the patched data chunk

    Every byte of dst outside the samples of the detected runs equals src: header, other chunks, the other channels' samples inside a run's
    frames, and a trailing partial frame.  A channel with more runs than `max_gaps` raises ValueError and nothing is written (count comes to
    the host once, for this check)."""
    from .wav_io import _data_tensor, decode_pcm, parse_wav, patch_pcm
    with open(src, "rb") as f:
        buf = f.read()
    info = parse_wav(buf)
    if info.frames < 1:
        raise ValueError("declick_file: %s holds no samples" % src)
    data = _data_tensor(buf, info, "cuda")
    wav = decode_pcm(data, info.fmt, info.channels)
    out, gaps, _ = declick(wav, **kwargs)
    K = gaps.start.size(1)
    over = (gaps.count > K).nonzero().flatten().tolist()
    if over:
        raise ValueError("declick_file: channels %s hold %s runs, the lists hold %d: detect with a larger max_gaps, k or merge_within"
                         % (over, [int(gaps.count[c]) for c in over], K))
    patched = patch_pcm(data, out, info.fmt, gaps).cpu().numpy().tobytes()
    end = info.data_offset + info.data_bytes
    with open(dst, "wb") as f:
        f.write(buf[:info.data_offset] + patched + buf[end:])
    return gaps, info
