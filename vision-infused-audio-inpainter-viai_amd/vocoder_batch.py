"""WaveNet training batches on the GPU: a list of (signal, mel) pairs of different lengths in, one padded batch out (reference: `collate_fn`,
Data_loaders/data_loader_utils.py:209-319, its `upsample_conditional_features` branch).

The reference assembles a batch on the host in numpy; here the pairs stay where `UtterancePreprocessor` left them, on the device, and one launch
(`viai_voc_collate`, csrc/vocoder_batch.hip) writes everything `WaveNet.forward_nhwc` and the masked losses consume.

    crop      rows longer than `max_time_steps` are cut to a random window on the frame grid (:226-249)                (crop_plan, on the host)
    pad       zero padding to the longest row of the batch (:273-297)                                                   (the kernel)
    inputs    one-hot (B, K, T) or float (B, 1, T); targets (B, T, 1); the class indices (B, T) `forward_nhwc` takes   (the kernel)
    mel       (N, D) -> (B, D, frames) (:296-300)                                                                       (the kernel)

Which utterances form a batch is the caller's choice: `PartialyRandomizedSimilarTimeLengthSampler` is not ported.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import torch

from . import _lib
from .audio import AudioConfig
from .preprocess import INPUT_TYPES

VocoderBatch = namedtuple("VocoderBatch", "x y c g input_lengths classes starts frames")
VocoderBatch.__doc__ = """One training batch.  T = max(frames) * hop (or `pad_to`), L = T / hop.
"mulaw-quantize": y (B, T, 1) int64 targets; classes (B, T) int32, the same numbers; x (B, K, T) fp32 one-hot with `one_hot=True`, else None.
"mulaw" / "raw": x (B, 1, T) fp32 and y (B, T, 1) fp32 -- two views of ONE buffer (same numbers, same order); classes None.
c (B, D, L) fp32 or None; g (B,) int64 or None; input_lengths (B,) int64 on the device; starts, frames: the crop plan, Python lists."""


def crop_plan(n_frames, hop, max_time_steps=None, max_time_sec=None, sample_rate=16000, rng=None, starts=None):
    """The crop of `collate_fn` (:226-249) for rows of `n_frames` mel frames (a list of ints) -> (starts, frames), two lists.

    max_time_steps = int(max_time_sec * sample_rate) when max_time_sec is given, else the argument; both None: no crop.  With
    max_steps = max_time_steps - max_time_steps % hop and L = max_steps // hop, a row with n * hop > max_steps (strictly) keeps L frames from
    start = rng.randint(0, n - L) on -- one draw per cropped row, in batch order; every other row keeps its n frames from 0.
    The high bound of the draw is EXCLUSIVE, as in the reference: the last window, start = n - L, is never drawn, and a row with n - L == 1
    always gets 0.  That is the reference's behaviour and is kept.  rng: a numpy.random.RandomState (None: a fresh one); `np.random.seed(k)` followed
    by the reference's calls draws what RandomState(k) draws.
    starts: the starts themselves instead of draws, one per row, each validated: 0 <= s <= n - L for a cropped row, 0 for any other.
    ValueError: an empty list, n < 1, hop < 1, L == 0 (max_time_steps < hop)."""
    hop = int(hop)
    if hop < 1:
        raise ValueError("crop_plan: hop >= 1")
    n_frames = [int(n) for n in n_frames]
    if not n_frames:
        raise ValueError("crop_plan: no row")
    if min(n_frames) < 1:
        raise ValueError("crop_plan: every row has at least one frame")
    if starts is not None:
        starts = [int(s) for s in starts]
        if len(starts) != len(n_frames):
            raise ValueError("crop_plan: %d starts for %d rows" % (len(starts), len(n_frames)))
    if max_time_sec is not None:
        max_time_steps = int(max_time_sec * sample_rate)
    L = None
    if max_time_steps is not None:
        max_steps = int(max_time_steps) - int(max_time_steps) % hop
        L = max_steps // hop
        if L < 1:
            raise ValueError("crop_plan: max_time_steps = %d is shorter than one frame of %d samples" % (max_time_steps, hop))
    out_s, out_f = [], []
    for i, n in enumerate(n_frames):
        keep = L if L is not None and n > L else n                    # n * hop > max_steps  <=>  n > L
        if starts is not None:
            s = starts[i]
            if not 0 <= s <= n - keep:
                raise ValueError("crop_plan: start %d of row %d is outside [0, %d]" % (s, i, n - keep))
        elif keep < n:
            if rng is None:
                rng = np.random.RandomState()
            s = int(rng.randint(0, n - keep))
        else:
            s = 0
        out_s.append(s)
        out_f.append(keep)
    return out_s, out_f


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _row(i, sig, mel, hop, sig_dtype, dev):
    """validate one pair -> its frame count"""
    what = "VocoderBatcher: row %d" % i
    for name, t in (("signal", sig), ("mel", mel)):
        if t is None and name == "mel":
            continue
        if not isinstance(t, torch.Tensor):
            raise ValueError("%s: %s is a tensor" % (what, name))
        if not t.is_cuda:
            raise _lib.ViaiLibraryError("%s: VocoderBatcher runs on the GPU only; no CPU fallback (%s is on %s)" % (what, name, t.device))
        if t.device != dev:
            raise ValueError("%s: %s is on %s, row 0 on %s" % (what, name, t.device, dev))
        if not t.is_contiguous():
            raise ValueError("%s: %s is contiguous" % (what, name))
    if sig.dtype != sig_dtype:
        raise TypeError("%s: signal is %s, got %s" % (what, sig_dtype, sig.dtype))
    if sig.dim() != 1 or sig.numel() < hop or sig.numel() % hop:
        raise ValueError("%s: signal holds N * hop samples (N >= 1, hop %d), got shape %s" % (what, hop, tuple(sig.shape)))
    n = sig.numel() // hop
    if mel is not None:
        if mel.dtype != torch.float32:
            raise TypeError("%s: mel is float32, got %s" % (what, mel.dtype))
        if mel.dim() != 2 or mel.shape[1] < 1:
            raise ValueError("%s: mel is (N, D)" % what)
        if mel.shape[0] * hop != sig.numel():                          # assert_ready_for_upsampling (:43-44)
            raise ValueError("%s: %d mel frames of %d samples do not cover the signal's %d samples" % (what, mel.shape[0], hop, sig.numel()))
    return n


class VocoderBatcher:
    """hop, sample_rate: None = `AudioConfig`'s.  input_type: "mulaw-quantize" (int32 class signals), "mulaw" or "raw" (float signals).
    max_time_steps / max_time_sec: the crop of `crop_plan`; both None: no crop.  one_hot: also write the dense (B, K, T) input the reference feeds
    ("mulaw-quantize" only, quantize_channels a multiple of 4).  pad_to: T = max(longest row, pad_to), rounded up to a multiple of hop -- batches of one
    fixed shape for captured steps.

    Padding is the reference's: targets and classes 0, float inputs 0.0, one-hot columns all zero at t >= length, c zero at frame >= frames[b].
    One consequence in class form: `forward_nhwc` gathers row 0 of the first conv at a padded position where the reference feeds a zero column.
    These positions lie after every valid sample of their row, the network is causal and the mask excludes them, so no masked-loss term and no
    gradient through a valid position differs.

    Not ported, each refused with a ValueError: upsample_conditional_features=False (`adjust_time_resolution`, :250-255), and the branch without
    local conditioning (:258-270), which trims silence and crops on the sample grid at collate time: pairs without a mel are taken only when no
    crop is configured, and as they are (`UtterancePreprocessor` has trimmed them already)."""

    def __init__(self, hop=None, input_type="mulaw-quantize", quantize_channels=256, max_time_steps=None, max_time_sec=None, sample_rate=None,
                 one_hot=False, pad_to=None, upsample_conditional_features=True):
        if input_type not in INPUT_TYPES:
            raise ValueError("VocoderBatcher: input_type is one of %s, not %r" % (", ".join(INPUT_TYPES), input_type))
        if not upsample_conditional_features:
            raise ValueError("VocoderBatcher: upsample_conditional_features=False (adjust_time_resolution) is not ported")
        self.hop = int(AudioConfig.hop_size if hop is None else hop)
        self.sample_rate = AudioConfig.sample_rate if sample_rate is None else sample_rate
        if self.hop < 1:
            raise ValueError("VocoderBatcher: hop >= 1")
        self.input_type, self.mode = input_type, INPUT_TYPES.index(input_type)
        self.K = int(quantize_channels)
        if self.mode == 0 and self.K < 2:
            raise ValueError("VocoderBatcher: quantize_channels >= 2")
        self.one_hot = bool(one_hot)
        if self.one_hot and (self.mode != 0 or self.K % 4):
            raise ValueError("VocoderBatcher: one_hot needs input_type \"mulaw-quantize\" and quantize_channels a multiple of 4")
        if pad_to is not None and int(pad_to) < 1:
            raise ValueError("VocoderBatcher: pad_to >= 1")
        self.pad_to = None if pad_to is None else int(pad_to)
        self.max_time_steps, self.max_time_sec = max_time_steps, max_time_sec
        if max_time_steps is not None or max_time_sec is not None:
            crop_plan([1], self.hop, max_time_steps, max_time_sec, self.sample_rate)      # refuses a crop shorter than one frame now
        self.crops = max_time_steps is not None or max_time_sec is not None

    def __call__(self, utterances, rng=None, starts=None, speaker_ids=None):
        """utterances: a list of `preprocess.Utterance` or of (signal, mel) tuples; mel (N, D) fp32 contiguous, or None for ALL rows; signal (N * hop,)
        contiguous, int32 for "mulaw-quantize" and fp32 otherwise, everything on one GPU.  rng / starts: see `crop_plan`.  speaker_ids: B ints -> g.
        One small host-to-device copy (the table of pointers, starts, frames, lengths and speaker ids, one tensor), one launch on the current
        stream, no device-to-host read and no synchronisation.  The sources are read by that launch: they are referenced by `utterances` until
        it is enqueued, which is all stream-ordered allocation needs."""
        rows = []
        for u in utterances:
            sig, mel = (u.signal, u.mel) if hasattr(u, "signal") else u
            rows.append((sig, mel))
        if not rows:
            raise ValueError("VocoderBatcher: no utterance")
        B, hop = len(rows), self.hop
        if B > 65535:
            raise ValueError("VocoderBatcher: at most 65535 rows")
        with_mel = rows[0][1] is not None
        if any((m is not None) != with_mel for _, m in rows):
            raise ValueError("VocoderBatcher: a mel for every row or for none")
        if not with_mel and self.crops:
            raise ValueError("VocoderBatcher: cropping pairs without local conditioning (trim and sample-grid crop at collate time) is not ported")
        dev = rows[0][0].device if isinstance(rows[0][0], torch.Tensor) else None
        sig_dtype = torch.int32 if self.mode == 0 else torch.float32
        n_frames = [_row(i, s, m, hop, sig_dtype, dev) for i, (s, m) in enumerate(rows)]
        D = 0
        if with_mel:
            D = int(rows[0][1].shape[1])
            if any(int(m.shape[1]) != D for _, m in rows):
                raise ValueError("VocoderBatcher: all mels share one D")
        if speaker_ids is not None:
            speaker_ids = [int(v) for v in speaker_ids]
            if len(speaker_ids) != B:
                raise ValueError("VocoderBatcher: %d speaker ids for %d rows" % (len(speaker_ids), B))
        st, fr = crop_plan(n_frames, hop, self.max_time_steps, self.max_time_sec, self.sample_rate, rng, starts)
        L = max(fr)
        if self.pad_to is not None:
            L = max(L, -(-self.pad_to // hop))
        T = L * hop
        if T > 2 ** 31 - 1:
            raise ValueError("VocoderBatcher: %d samples a row do not fit the kernel's int32 indices" % T)
        lib = _lib.load()
        # one table, one copy: int64 rows [signal pointers | mel pointers | starts and frames as int32 | lengths | speaker ids]
        ints = np.asarray(st + fr, dtype=np.int32).view(np.int64).tolist()
        tab = torch.tensor([s.data_ptr() for s, _ in rows] + [m.data_ptr() if with_mel else 0 for _, m in rows] + ints + [f * hop for f in fr] +
                           (speaker_ids or []), dtype=torch.int64).to(dev, non_blocking=True)
        base = tab.data_ptr()
        K = self.K
        x = c = classes = None
        if self.mode == 0:
            y = torch.empty((B, T, 1), dtype=torch.int64, device=dev)
            classes = torch.empty((B, T), dtype=torch.int32, device=dev)
            if self.one_hot:
                x = torch.empty((B, K, T), dtype=torch.float32, device=dev)
            y_ptr, x_ptr = y.data_ptr(), 0 if x is None else x.data_ptr()
        else:
            buf = torch.empty(B * T, dtype=torch.float32, device=dev)
            x, y = buf.view(B, 1, T), buf.view(B, T, 1)
            y_ptr, x_ptr = buf.data_ptr(), 0
        if with_mel:
            c = torch.empty((B, D, L), dtype=torch.float32, device=dev)
        _lib.check(lib.viai_voc_collate(base, base + 8 * B if with_mel else 0, base + 16 * B, base + 16 * B + 4 * B, B, hop, D, self.mode, K, T, L, y_ptr,
                                        0 if classes is None else classes.data_ptr(), x_ptr, 0 if c is None else c.data_ptr(), _stream()),
                   "viai_voc_collate")
        lengths = tab[3 * B:4 * B]
        g = tab[4 * B:5 * B] if speaker_ids is not None else None
        return VocoderBatch(x, y, c, g, lengths, classes, st, fr)
