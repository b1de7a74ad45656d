"""Short gaps filled without a network: Burg autoregressive interpolation on the device (csrc/ar_fill.hip).

    ar_fill        every listed gap of every row of a batch, one launch -> (out, filled)
    ar_fill_host   the same rule on numpy arrays, in plain C++ on the host (`viai_ar_fill_host`): no GPU needed
    ar_fit_host    the Burg fit alone on one numpy vector (`viai_ar_fit_host`): coefficients and order
    janssen_fill, janssen_fill_host, janssen_plan_host   re-exported from `viai_amd.janssen`: dense runs (crackle) solved jointly per window

The rule (include/viai_hip.h states it in full, csrc/viai_ar_rule.h is its arithmetic): an all-pole model is fitted to the clean samples on
each side of a gap, extrapolated into it from both sides, and the two predictions are cross-faded.  fp64, + - * / only, every sum in a fixed
order: the same bits on the host and on the device, from run to run, and for a row alone or in any batch.

`filled` codes: 1 both sides, 2 left only, 3 right only, 4 no context (zeros written), 0 skipped (not listed, empty, longer than max_len, or
outside the row).
"""
from __future__ import annotations

import torch

from . import _lib
from .janssen import janssen_fill, janssen_fill_host, janssen_plan_host  # noqa: F401

MAX_ORDER, MAX_CONTEXT, MAX_LEN = 128, 4096, 4096          # AR_MAX_* of csrc/viai_ar_rule.h


def _limits(what, order, context, max_len):
    if int(order) != order or int(context) != context or int(max_len) != max_len:
        raise ValueError("%s: order, context and max_len are integers" % what)
    if not (1 <= order <= MAX_ORDER and 2 <= context <= MAX_CONTEXT and 1 <= max_len <= MAX_LEN):
        raise ValueError("%s: 1 <= order <= %d, 2 <= context <= %d, 1 <= max_len <= %d" % (what, MAX_ORDER, MAX_CONTEXT, MAX_LEN))
    return int(order), int(context), int(max_len)


def ar_fill(wav, gaps, lengths=None, order=32, context=1024, max_len=4096):
    """wav (B, n) fp32 on the GPU, any B >= 1 and n >= 1; gaps a `Gaps` (or 3-tuple) of int32 count (B,), start (B, K), length (B, K).
    Returns (out, filled): out a clone of wav with the samples of the filled gaps replaced, filled (B, K) int32 codes, both on wav's device.

    lengths   (B,) ints, a tensor on either side or a sequence: row b holds clamp(lengths[b], 0, n) samples; a gap that crosses the end is
              skipped, a context stops there.
    order     the model order per side; a side with C context samples uses min(order, C // 2).
    context   how many clean samples each side may use; it stops early at a neighbouring listed gap and at the row's ends.
    max_len   longer gaps are skipped (filled = 0).

    One launch, no synchronisation.  Gaps that are int32, contiguous and already on wav's device are read where they lie: nothing is
    copied.  A wav that is not fp32 or whose rows are not contiguous is converted by the clone.  ViaiLibraryError for a CPU tensor: no CPU
    fallback (`ar_fill_host` is the host's call)."""
    order, context, max_len = _limits("ar_fill", order, context, max_len)
    if wav.dim() != 2 or wav.size(0) < 1 or wav.size(1) < 1:
        raise ValueError("ar_fill: wav is (B, n)")
    B, n = wav.shape
    if n >= 2 ** 31:
        raise ValueError("ar_fill: %d samples per row; fewer than 2^31" % n)
    count, start, length = (torch.as_tensor(x) for x in tuple(gaps))
    if count.dim() != 1 or count.numel() != B or start.dim() != 2 or start.size(0) != B or start.size(1) < 1 or start.shape != length.shape:
        raise ValueError("ar_fill: gaps are (count (B,), start (B, K), length (B, K)) with B = %d, K >= 1" % B)
    if lengths is not None:
        lengths = torch.as_tensor(lengths).reshape(-1)
        if lengths.numel() != B:
            raise ValueError("ar_fill: lengths holds one entry per row (B = %d)" % B)
    if not wav.is_cuda:
        raise _lib.ViaiLibraryError("ar_fill runs on the GPU only; no CPU fallback (ar_fill_host states the rule on the host)")
    lib = _lib.load()
    from .ops import _stream
    dev = wav.device
    K = start.size(1)
    out = wav.float().clone(memory_format=torch.contiguous_format)
    count, start, length = (x.to(device=dev, dtype=torch.int32).contiguous() for x in (count, start, length))       # no-ops when already so
    if lengths is not None:
        lengths = lengths.to(dev).clamp(-1, 0x7fffffff).to(torch.int32).contiguous()
    filled = torch.empty(B, K, dtype=torch.int32, device=dev)
    # the kernel reads its contexts from `out` itself: they hold no sample of a listed gap, so they are wav's samples
    _lib.check(lib.viai_ar_fill(out.data_ptr(), 0 if lengths is None else lengths.data_ptr(), n, B, n, count.data_ptr(), start.data_ptr(),
                                length.data_ptr(), K, order, context, max_len, out.data_ptr(), n, filled.data_ptr(), _stream()), "viai_ar_fill")
    return out, filled


def ar_fill_host(wav, gaps, lengths=None, order=32, context=1024, max_len=4096):
    """`ar_fill` on the host: wav a (B, n) numpy array (a view of wider rows is read in place), gaps three integer arrays.  Returns
    (out, filled) as numpy arrays, out a contiguous fp32 copy of wav with the filled samples replaced.  Needs the built library, not a GPU."""
    import ctypes as C

    import numpy as np
    order, context, max_len = _limits("ar_fill_host", order, context, max_len)
    wav = np.asarray(wav, dtype=np.float32)
    if wav.ndim != 2 or wav.shape[0] < 1 or wav.shape[1] < 1:
        raise ValueError("ar_fill_host: wav is (B, n)")
    B, n = wav.shape
    if n >= 2 ** 31:
        raise ValueError("ar_fill_host: %d samples per row; fewer than 2^31" % n)
    if wav.strides[1] != 4 or wav.strides[0] % 4 != 0 or wav.strides[0] < 4 * n:
        wav = np.ascontiguousarray(wav)
    stride = wav.strides[0] // 4
    count, start, length = (np.ascontiguousarray(np.asarray(x), dtype=np.int32) for x in tuple(gaps))
    if count.ndim != 1 or count.size != B or start.ndim != 2 or start.shape[0] != B or start.shape[1] < 1 or start.shape != length.shape:
        raise ValueError("ar_fill_host: gaps are (count (B,), start (B, K), length (B, K)) with B = %d, K >= 1" % B)
    K = start.shape[1]
    lp = None
    if lengths is not None:
        lengths = np.ascontiguousarray(np.clip(np.asarray(lengths, dtype=np.int64).reshape(-1), -1, 0x7fffffff), dtype=np.int32)
        if lengths.size != B:
            raise ValueError("ar_fill_host: lengths holds one entry per row (B = %d)" % B)
        lp = lengths.ctypes.data_as(C.c_void_p)
    out = np.array(wav, dtype=np.float32, order="C", copy=True)
    filled = np.empty((B, K), dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    _lib.check(_lib.load().viai_ar_fill_host(p(wav), lp, stride, B, n, p(count), p(start), p(length), K, order, context, max_len, p(out), n,
                                             p(filled)), "viai_ar_fill_host")
    return out, filled


def ar_fit_host(x, order):
    """Burg's fit of the rule on one vector x (C,), 0 <= C <= 4096: returns (a, p), a the order + 1 fp64 coefficients (a[0] = 1, zeros behind
    a[p]) and p = min(order, C // 2).  Needs the built library, not a GPU."""
    import ctypes as C

    import numpy as np
    if int(order) != order or not 1 <= order <= MAX_ORDER:
        raise ValueError("ar_fit_host: 1 <= order <= %d" % MAX_ORDER)
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float32))
    if x.ndim != 1 or x.size > MAX_CONTEXT:
        raise ValueError("ar_fit_host: x is (C,) with C <= %d" % MAX_CONTEXT)
    a = np.empty(int(order) + 1, dtype=np.float64)
    p = C.c_int(0)
    _lib.check(_lib.load().viai_ar_fit_host(x.ctypes.data_as(C.c_void_p), x.size, int(order), a.ctypes.data_as(C.c_void_p), C.byref(p)),
               "viai_ar_fit_host")
    return a, p.value
