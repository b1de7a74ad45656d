"""Crackle and short gaps filled jointly: Janssen's least-squares AR interpolation on the device (csrc/janssen_fill.hip).

    janssen_fill        every cluster of listed runs of every row of a batch, one launch -> (out, filled)
    janssen_fill_host   the same rule on numpy arrays, in plain C++ on the host (`viai_janssen_fill_host`): no GPU needed
    janssen_plan_host   the cluster rule alone (`viai_janssen_plan_host`): per entry its leader, window and number of unknowns

The rule (include/viai_hip.h states it in full, csrc/viai_janssen_rule.h is its arithmetic): listed runs that lie within `context` of each
other form a cluster; one all-pole model is fitted (Burg, the fit of `ar_fill`) to the cluster's whole window with the current estimates in
place, all its missing samples are solved for jointly from the banded normal equations (L D L^T), and that is repeated `iters` times.  fp64,
+ - * / only, every sum in a fixed order: the same bits on the host and on the device, from run to run, and for a row alone or in any batch.

`filled` codes, the same for every member of a cluster: 1 solved for all iters, 4 no model (a window of fewer than 2 samples; zeros written),
5 stopped at a pivot that was not positive (the last completed iteration's estimates are written, zeros if none), 0 skipped (not listed,
empty, longer than max_len, outside the row, or in front of the end of an earlier entry).  THERE IS NO FALLBACK to `ar_fill` for the entries
skipped here: `filled` says which they are, and the caller decides.
"""
from __future__ import annotations

import torch

from . import _lib

MAX_ORDER, MAX_CONTEXT, MAX_ITERS = 128, 1024, 16          # AR_MAX_ORDER, JN_MAX_CONTEXT, JN_MAX_ITERS
MAX_UNKNOWN, BAND_DOUBLES, MAX_WINDOW = 1024, 8192, 4096   # JN_* of csrc/viai_janssen_rule.h


def rule_max_len(order, context):
    """the largest max_len the rule allows: min(1024, 8192 // (order + 1), 4096 - 2 context)"""
    return min(MAX_UNKNOWN, BAND_DOUBLES // (int(order) + 1), MAX_WINDOW - 2 * int(context))


def _limits(what, order, context, iters, max_len):
    if int(order) != order or int(context) != context or int(iters) != iters or (max_len is not None and int(max_len) != max_len):
        raise ValueError("%s: order, context, iters and max_len are integers" % what)
    if not (1 <= order <= MAX_ORDER and 2 <= context <= MAX_CONTEXT and 1 <= iters <= MAX_ITERS):
        raise ValueError("%s: 1 <= order <= %d, 2 <= context <= %d, 1 <= iters <= %d" % (what, MAX_ORDER, MAX_CONTEXT, MAX_ITERS))
    top = rule_max_len(order, context)
    if max_len is None:
        max_len = top
    if not 1 <= max_len <= top:
        raise ValueError("%s: 1 <= max_len <= %d at order %d and context %d" % (what, top, order, context))
    return int(order), int(context), int(iters), int(max_len)


def janssen_fill(wav, gaps, lengths=None, order=32, context=1024, iters=3, max_len=None):
    """wav (B, n) fp32 on the GPU, any B >= 1 and n >= 1; gaps a `Gaps` (or 3-tuple) of int32 count (B,), start (B, K), length (B, K).
    Returns (out, filled): out a clone of wav with the samples of the solved runs replaced, filled (B, K) int32 codes, both on wav's device.

    lengths   (B,) ints, a tensor on either side or a sequence: row b holds clamp(lengths[b], 0, n) samples; a run that crosses the end is
              skipped, a window stops there.
    order     the model order; a window of W samples uses min(order, W // 2).
    context   how many samples a window reaches beyond its first and last run, and how close runs must lie to be solved together; a
              window stops early at a run of another cluster, at a skipped entry and at the row's ends.
    iters     fit-and-solve rounds (1 .. 16); single gaps have converged after 2.
    max_len   longer runs are skipped (filled = 0).  None: the largest the rule allows, `rule_max_len(order, context)`.

    One launch, no synchronisation.  Gaps that are int32, contiguous and already on wav's device (as `find_clicks` and `find_gaps` leave
    them) are read where they lie: nothing is copied.  ValueError for an argument outside its limits, before anything is launched.
    ViaiLibraryError for a CPU tensor: no CPU fallback (`janssen_fill_host` is the host's call).  No fallback to `ar_fill` for skipped
    entries either: see `filled`."""
    order, context, iters, max_len = _limits("janssen_fill", order, context, iters, max_len)
    if wav.dim() != 2 or wav.size(0) < 1 or wav.size(1) < 1:
        raise ValueError("janssen_fill: wav is (B, n)")
    B, n = wav.shape
    if n >= 2 ** 31:
        raise ValueError("janssen_fill: %d samples per row; fewer than 2^31" % n)
    count, start, length = (torch.as_tensor(x) for x in tuple(gaps))
    if count.dim() != 1 or count.numel() != B or start.dim() != 2 or start.size(0) != B or start.size(1) < 1 or start.shape != length.shape:
        raise ValueError("janssen_fill: gaps are (count (B,), start (B, K), length (B, K)) with B = %d, K >= 1" % B)
    if lengths is not None:
        lengths = torch.as_tensor(lengths).reshape(-1)
        if lengths.numel() != B:
            raise ValueError("janssen_fill: lengths holds one entry per row (B = %d)" % B)
    if not wav.is_cuda:
        raise _lib.ViaiLibraryError("janssen_fill runs on the GPU only; no CPU fallback (janssen_fill_host states the rule on the host)")
    lib = _lib.load()
    from .ops import _stream
    dev = wav.device
    K = start.size(1)
    out = wav.float().clone(memory_format=torch.contiguous_format)
    count, start, length = (x.to(device=dev, dtype=torch.int32).contiguous() for x in (count, start, length))       # no-ops when already so
    if lengths is not None:
        lengths = lengths.to(dev).clamp(-1, 0x7fffffff).to(torch.int32).contiguous()
    filled = torch.empty(B, K, dtype=torch.int32, device=dev)
    # the kernel reads its windows from `out` itself: a window holds no unknown of another cluster, so what it reads are wav's samples
    _lib.check(lib.viai_janssen_fill(out.data_ptr(), 0 if lengths is None else lengths.data_ptr(), n, B, n, count.data_ptr(), start.data_ptr(),
                                     length.data_ptr(), K, order, context, max_len, iters, out.data_ptr(), n, filled.data_ptr(), _stream()),
               "viai_janssen_fill")
    return out, filled


def _host_lists(what, B, gaps, lengths):
    import ctypes as C

    import numpy as np
    count, start, length = (np.ascontiguousarray(np.asarray(x), dtype=np.int32) for x in tuple(gaps))
    if count.ndim != 1 or count.size != B or start.ndim != 2 or start.shape[0] != B or start.shape[1] < 1 or start.shape != length.shape:
        raise ValueError("%s: gaps are (count (B,), start (B, K), length (B, K)) with B = %d, K >= 1" % (what, B))
    if lengths is not None:
        lengths = np.ascontiguousarray(np.clip(np.asarray(lengths, dtype=np.int64).reshape(-1), -1, 0x7fffffff), dtype=np.int32)
        if lengths.size != B:
            raise ValueError("%s: lengths holds one entry per row (B = %d)" % (what, B))
    return count, start, length, lengths, (None if lengths is None else lengths.ctypes.data_as(C.c_void_p))


def janssen_fill_host(wav, gaps, lengths=None, order=32, context=1024, iters=3, max_len=None):
    """`janssen_fill` on the host: wav a (B, n) numpy array (a view of wider rows is read in place), gaps three integer arrays.  Returns
    (out, filled) as numpy arrays, out a contiguous fp32 copy of wav with the solved samples replaced.  Needs the built library, not a GPU."""
    import ctypes as C

    import numpy as np
    order, context, iters, max_len = _limits("janssen_fill_host", order, context, iters, max_len)
    wav = np.asarray(wav, dtype=np.float32)
    if wav.ndim != 2 or wav.shape[0] < 1 or wav.shape[1] < 1:
        raise ValueError("janssen_fill_host: wav is (B, n)")
    B, n = wav.shape
    if n >= 2 ** 31:
        raise ValueError("janssen_fill_host: %d samples per row; fewer than 2^31" % n)
    if wav.strides[1] != 4 or wav.strides[0] % 4 != 0 or wav.strides[0] < 4 * n:
        wav = np.ascontiguousarray(wav)
    stride = wav.strides[0] // 4
    count, start, length, lengths, lp = _host_lists("janssen_fill_host", B, gaps, lengths)
    K = start.shape[1]
    out = np.array(wav, dtype=np.float32, order="C", copy=True)
    filled = np.empty((B, K), dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    _lib.check(_lib.load().viai_janssen_fill_host(p(wav), lp, stride, B, n, p(count), p(start), p(length), K, order, context, max_len, iters,
                                                  p(out), n, p(filled)), "viai_janssen_fill_host")
    return out, filled


def janssen_plan_host(n, gaps, lengths=None, order=32, context=1024, max_len=None):
    """The cluster rule alone for rows of n samples: returns (leader, lo, hi, unknowns), four (B, K) int32 numpy arrays.  leader[b, k] is the
    index of the first member of entry k's cluster, -1 for a skipped entry (the other three are then 0); [lo, hi) is the cluster's window and
    unknowns its M.  Needs the built library, not a GPU."""
    import ctypes as C

    import numpy as np
    order, context, _, max_len = _limits("janssen_plan_host", order, context, 1, max_len)
    if int(n) != n or not 1 <= n < 2 ** 31:
        raise ValueError("janssen_plan_host: 1 <= n < 2^31")
    B = int(np.asarray(tuple(gaps)[0]).size)
    count, start, length, lengths, lp = _host_lists("janssen_plan_host", B, gaps, lengths)
    K = start.shape[1]
    res = tuple(np.empty((B, K), dtype=np.int32) for _ in range(4))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    _lib.check(_lib.load().viai_janssen_plan_host(lp, B, int(n), p(count), p(start), p(length), K, order, context, max_len, *(p(r) for r in res)),
               "viai_janssen_plan_host")
    return res
