"""Where a waveform is damaged, found on the device (csrc/gap_detect.hip), and `repair`: detect, then inpaint.

    find_gaps        runs of non-finite, silent or clipped samples of every row of a batch -> Gaps(count, start, length) on the device
    find_gaps_host   the same rule on a numpy array, in plain C++ on the host (`viai_gap_detect_host`): no GPU needed
    repair           `find_gaps` + one `AudioInpainter` call per gap index; with `ar_below`, gaps shorter than that go to `ar_fill` first

The rule (include/viai_hip.h states it in full): a sample is damaged when it is not finite, or |x| <= threshold, or (clip > 0 and |x| >= clip).
Maximal runs of damaged samples inside a row's length are kept when they are at least `min_len` long; kept runs at most `merge_within` samples
apart join into one.  The results are integers and exact: the same bits from run to run, and for a row alone or in any batch.

A clip at another sample rate: `repair(..., sample_rate=...)` detects on the clip itself and runs every pass through `inpaint_at_rate`.
"""
from __future__ import annotations

from collections import namedtuple

import torch

from . import _lib

Gaps = namedtuple("Gaps", ("count", "start", "length"))
Gaps.__doc__ = """count (B,), start (B, K), length (B, K), int32.  count[b] is the true number of gaps of row b and may exceed K; start / length hold
the first K in position order and are 0 from entry min(count[b], K) on."""

TILE = 4096                                              # VIAI_GAP_DETECT_TILE of include/viai_hip.h: the samples one block owns


def _rule(what, threshold, clip, min_len, merge_within, max_gaps):
    if int(min_len) != min_len or int(merge_within) != merge_within or int(max_gaps) != max_gaps:
        raise ValueError("%s: min_len, merge_within and max_gaps are integers" % what)
    if min_len < 1 or merge_within < 0 or max_gaps < 1 or max(min_len, merge_within, max_gaps) > 0x7fffffff:
        raise ValueError("%s: min_len >= 1, merge_within >= 0, max_gaps >= 1" % what)
    if not float(threshold) >= 0.0 or not float(clip) >= 0.0:
        raise ValueError("%s: threshold >= 0 and clip >= 0 (clip = 0: no clipping test)" % what)
    return float(threshold), float(clip), int(min_len), int(merge_within), int(max_gaps)


def find_gaps(wav, lengths=None, threshold=0.0, clip=0.0, min_len=64, merge_within=0, max_gaps=16):
    """wav (B, n) fp32 on the GPU -> Gaps(count, start, length), int32 tensors on wav's device, K = max_gaps.

    lengths       (B,) ints, a tensor on either side or a sequence: row b holds clamp(lengths[b], 0, n) samples; what lies behind neither starts
                  nor extends a run.
    threshold     |x| <= threshold is damaged; the default 0 means exact zeros (-0.0 included).
    clip          |x| >= clip is damaged; 0 switches the test off.  Non-finite samples are always damaged.
    min_len       shorter runs are dropped.  The default 64 is a CHOICE, not a measurement: speech decoded from int16 has short natural runs of
                  exact zeros, and 64 samples (4 ms at 16 kHz) is longer than those and shorter than a lost packet.
    merge_within  kept runs at most this many samples apart join (the distance is between kept runs; dropped runs in between do not count).

    Three launches for the batch, no synchronisation, and no copy to the host.  The workspace (1 bit per sample and 52 bytes per 4096-sample
    tile) is ALLOCATED PER CALL from torch's caching allocator, like the other modules' workspaces; nothing is cached here.  A wav that is not
    fp32 or whose rows are not contiguous is converted first (a copy).  ViaiLibraryError for a CPU tensor: no CPU fallback (`find_gaps_host` is
    the host's call)."""
    threshold, clip, min_len, merge_within, K = _rule("find_gaps", threshold, clip, min_len, merge_within, max_gaps)
    if wav.dim() != 2 or wav.size(0) < 1 or wav.size(1) < 1:
        raise ValueError("find_gaps: wav is (B, n)")
    B, n = wav.shape
    if n >= 2 ** 31:
        raise ValueError("find_gaps: %d samples per row; fewer than 2^31" % n)
    if lengths is not None:
        lengths = torch.as_tensor(lengths).reshape(-1)
        if lengths.numel() != B:
            raise ValueError("find_gaps: lengths holds one entry per row (B = %d)" % B)
    if not wav.is_cuda:
        raise _lib.ViaiLibraryError("find_gaps runs on the GPU only; no CPU fallback (find_gaps_host states the rule on the host)")
    lib = _lib.load()
    from .ops import _stream
    wav = wav.float()
    if wav.stride(1) != 1 or (B > 1 and wav.stride(0) < n):
        wav = wav.contiguous()
    dev = wav.device
    stride = wav.stride(0) if B > 1 else n
    if lengths is not None:
        lengths = lengths.to(dev).clamp(-1, 0x7fffffff).to(torch.int32).contiguous()
    nbytes = int(lib.viai_gap_detect_ws_bytes(B, n, K))
    if nbytes < 1:
        raise ValueError("find_gaps: no launch geometry for B = %d, n = %d" % (B, n))
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
    count = torch.empty(B, dtype=torch.int32, device=dev)
    start = torch.empty(B, K, dtype=torch.int32, device=dev)
    length = torch.empty(B, K, dtype=torch.int32, device=dev)
    _lib.check(lib.viai_gap_detect(wav.data_ptr(), 0 if lengths is None else lengths.data_ptr(), stride, B, n, threshold, clip, min_len,
                                   merge_within, K, count.data_ptr(), start.data_ptr(), length.data_ptr(), ws.data_ptr(), _stream()),
               "viai_gap_detect")
    return Gaps(count, start, length)


def find_gaps_host(wav, lengths=None, threshold=0.0, clip=0.0, min_len=64, merge_within=0, max_gaps=16):
    """`find_gaps` on the host: wav a (B, n) numpy array (or anything numpy makes one of), the rule stated sample by sample in plain C++
    (`viai_gap_detect_host`).  Returns Gaps of int32 numpy arrays.  Needs the built library, not a GPU."""
    import ctypes as C

    import numpy as np
    threshold, clip, min_len, merge_within, K = _rule("find_gaps_host", threshold, clip, min_len, merge_within, max_gaps)
    wav = np.asarray(wav, dtype=np.float32)
    if wav.ndim != 2 or wav.shape[0] < 1 or wav.shape[1] < 1:
        raise ValueError("find_gaps_host: wav is (B, n)")
    B, n = wav.shape
    if wav.strides[1] != 4 or wav.strides[0] % 4 != 0 or wav.strides[0] < 4 * n:           # a view of wider rows is read in place
        wav = np.ascontiguousarray(wav)
    stride = wav.strides[0] // 4
    if n >= 2 ** 31:
        raise ValueError("find_gaps_host: %d samples per row; fewer than 2^31" % n)
    lp = 0
    if lengths is not None:
        lengths = np.ascontiguousarray(np.clip(np.asarray(lengths, dtype=np.int64).reshape(-1), -1, 0x7fffffff), dtype=np.int32)
        if lengths.size != B:
            raise ValueError("find_gaps_host: lengths holds one entry per row (B = %d)" % B)
        lp = lengths.ctypes.data_as(C.c_void_p)
    count = np.empty(B, dtype=np.int32)
    start = np.empty((B, K), dtype=np.int32)
    length = np.empty((B, K), dtype=np.int32)
    _lib.check(_lib.load().viai_gap_detect_host(wav.ctypes.data_as(C.c_void_p), lp, stride, B, n, threshold, clip, min_len, merge_within, K,
                                                count.ctypes.data_as(C.c_void_p), start.ctypes.data_as(C.c_void_p),
                                                length.ctypes.data_as(C.c_void_p)), "viai_gap_detect_host")
    return Gaps(count, start, length)


def _without_filled(count, start, length, filled):
    """the host lists with the entries whose `filled` code is 1 .. 4 taken out and the rest moved to the front, zeros behind"""
    B, K = start.shape
    count, start, length = count.clone(), start.clone(), length.clone()
    for b in range(B):
        keep = [k for k in range(int(count[b])) if int(filled[b, k]) == 0]
        if len(keep) == int(count[b]):
            continue
        s, l = start[b, keep].clone(), length[b, keep].clone()
        start[b], length[b] = 0, 0
        start[b, :len(keep)], length[b, :len(keep)] = s, l
        count[b] = len(keep)
    return count, start, length


def repair(inpainter, wav, gaps=None, uniforms=None, fade=0, sample_rate=None, ar_below=0, ar_order=32, ar_context=1024, ar_lengths=None,
           ar_method="burg", ar_iters=None, **find_gaps_kwargs):
    """Detect the gaps of wav (B, n) and regenerate them with `inpainter` (an `AudioInpainter`).  Returns (waveform, Gaps).

    gaps       a `Gaps` from an earlier `find_gaps` (tensors or arrays); without it `find_gaps(wav, **find_gaps_kwargs)` runs.
    uniforms   a sequence with one entry per pass, each what `AudioInpainter.__call__` takes as `uniforms`; None: the sampler draws its own.
    fade       handed to every pass.
    sample_rate  None (the default): wav is at the front end's rate and `inpainter` is called directly, exactly as before this argument existed.
               A rate: pass k is `inpaint_at_rate(inpainter, wav, sample_rate, start[:, k], length[:, k], ...)`, which calls the inpainter
               directly when the rate is the front end's; the overflow rule and the single copy of the lists to the host are the same.
    ar_below   0 (the default): every gap goes to the inpainter, exactly as before this argument existed.  A length: gaps SHORTER than
               ar_below samples are filled first by one `ar_fill` launch (Burg autoregressive interpolation, `viai_amd.ar_fill`; order
               ar_order, context ar_context, max_len = min(ar_below - 1, 4096)) from the host copy of the lists; the entries it filled
               (`filled` 1 .. 4, read back once) leave the lists, the rest move to the front, and the passes below run over what remains, on
               a clip whose short gaps already hold plausible signal.  When nothing remains no pass runs, `inpainter` may be None and its
               limits on rows and hops do not apply.  ar_lengths: (B,) row lengths for `ar_fill` (contexts stop there); default: the
               `lengths` the detection was given, else n.
    ar_method  "burg" (the default): `ar_fill` as above.  "janssen": one `janssen_fill` launch instead (`viai_amd.janssen`: runs within
               ar_context of each other solved jointly, ar_iters rounds, default 3; ar_context at most 1024), with
               max_len = min(ar_below - 1, the rule's limit for ar_order and ar_context).  Entries that come back 0 go to the inpainter as
               above: there is no fallback from one autoregressive method to the other.

    count, start and length come to the host ONCE (one synchronisation).  If any row has more gaps than the lists hold (count > K) a ValueError
    names the rows and nothing is repaired: an overflowing detection is never half repaired.  Then pass k = 0 .. max(count) - 1 calls
    `inpainter(wav, start[:, k], length[:, k], uniforms=uniforms[k], fade=fade)` on the result of the pass before; rows with fewer gaps pass length 0,
    which the inpainter documents as "no gap".  When no row has a gap no pass runs and the result has wav's bits.  Every sample outside the
    detected gaps keeps its bits.

    The inpainter's limits are inherited and its errors pass through: 1, 2, 4 or 8 rows, n a whole number of hops, the generator's width rule.

    KNOWN LIMIT: while gap k of a clip is filled, the gaps to its right in the same clip are still damaged, and the frames they touch reach the
    generator and the vocoder's conditioning as if they were known.  Removing that needs several gaps per stream inside `AudioInpainter`."""
    if wav.dim() != 2:
        raise ValueError("repair: wav is (B, n)")
    B = wav.size(0)
    if int(ar_below) != ar_below or ar_below < 0:
        raise ValueError("repair: ar_below is a length in samples, 0 for no autoregressive fill")
    if ar_method not in ("burg", "janssen") or (ar_method == "burg" and ar_iters is not None):
        raise ValueError("repair: ar_method is 'burg' or 'janssen', and ar_iters belongs to 'janssen'")
    if gaps is None:
        gaps = find_gaps(wav, **find_gaps_kwargs)
        if ar_lengths is None:
            ar_lengths = find_gaps_kwargs.get("lengths")
    elif find_gaps_kwargs:
        raise ValueError("repair: gaps given, so nothing is detected: %s unused" % ", ".join(sorted(find_gaps_kwargs)))
    gaps = Gaps(*gaps)
    count, start, length = (torch.as_tensor(x) for x in gaps)
    if count.dim() != 1 or count.numel() != B or start.dim() != 2 or start.size(0) != B or start.shape != length.shape:
        raise ValueError("repair: gaps are (count (B,), start (B, K), length (B, K)) with B = %d" % B)
    K = start.size(1)
    packed = torch.cat((count.reshape(B, 1).to(torch.int64), start.to(torch.int64), length.to(torch.int64)), 1).cpu()      # the one copy
    count, start, length = packed[:, 0], packed[:, 1:1 + K], packed[:, 1 + K:]
    over = (count > K).nonzero().flatten().tolist()
    if over:
        raise ValueError("repair: rows %s hold %s gaps, the lists hold %d: detect with a larger max_gaps, min_len or merge_within"
                         % (over, [int(count[b]) for b in over], K))
    out = wav
    filled_any = False
    if ar_below > 1 and B > 0 and K > 0 and int(count.max()) > 0:
        lists = (count.to(torch.int32), start.to(torch.int32), length.to(torch.int32))
        if ar_method == "janssen":
            from .janssen import janssen_fill, rule_max_len
            out, filled = janssen_fill(wav, lists, lengths=ar_lengths, order=ar_order, context=ar_context,
                                       iters=3 if ar_iters is None else ar_iters,
                                       max_len=min(int(ar_below) - 1, max(rule_max_len(ar_order, ar_context), 1)))
        else:
            from .ar_fill import MAX_LEN, ar_fill
            out, filled = ar_fill(wav, lists, lengths=ar_lengths, order=ar_order, context=ar_context, max_len=min(int(ar_below) - 1, MAX_LEN))
        count, start, length = _without_filled(count, start, length, filled.cpu())
        filled_any = True
    passes = int(count.max()) if B > 0 else 0
    if passes > 0 and inpainter is None:
        left = {b: [int(v) for v in length[b, :int(count[b])]] for b in range(B) if int(count[b]) > 0}
        raise ValueError("repair: no inpainter, and rows %s still hold gaps of %s samples: pass an inpainter or a larger ar_below"
                         % (sorted(left), [left[b] for b in sorted(left)]))
    if uniforms is not None and len(uniforms) < passes:
        raise ValueError("repair: %d passes, uniforms for %d" % (passes, len(uniforms)))
    for k in range(passes):
        u = None if uniforms is None else uniforms[k]
        if sample_rate is None:
            out = inpainter(out, start[:, k].contiguous(), length[:, k].contiguous(), uniforms=u, fade=fade)
        else:
            from .wav_resample import inpaint_at_rate
            out = inpaint_at_rate(inpainter, out, sample_rate, start[:, k].contiguous(), length[:, k].contiguous(), uniforms=u, fade=fade)
    if passes == 0 and not filled_any:
        out = wav.float().clone()
    return out, gaps
