"""Vocoder data preparation on the GPU: a waveform in, (signal, mel) training pairs out (reference: `_process_utterance`, utils/librivox.py:44-117).

The reference prepares its vocoder's training set offline on the host (nnmnkwii, lws, librosa).  Here the stage runs on the device and computes the
mel with the front end `AudioInpainter` conditions the vocoder with (`MelFrontEnd`), on the same frame grid, so training and inference see mels from
one program.  Decoding the audio file stays on the host: the input is the decoded waveform.

    chunks     the file is cut into `chunk_samples` pieces, the last one running to the end of the file (librivox.py:56-63)    (chunk_bounds)
    rescale    x / max|x| * rescaling_max in fp32, as numpy does it (librivox.py:48-49)                     (viai_absmax, then inside both kernels)
    trim       `mulaw-quantize` only: first / last sample whose mu-law class is more than `silence_threshold` away from 127; the backward search
               never looks at samples 0 and 1 and the slice excludes the last active sample (utils/audio.py:56-67)      (viai_utt_trim_bounds)
    signal     l = fft - hop pad values, the trimmed signal, pad values up to N * hop, N = lws_num_frames (librivox.py:92-102)   (viai_utt_pack)
    mel        the front end on the trimmed, rescaled waveform, stored (N, num_mels)                                            (MelFrontEnd)
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import torch

from . import _lib
from .audio import AudioConfig, MelFrontEnd, lws_num_frames, lws_pad_lr

INPUT_TYPES = ("mulaw-quantize", "mulaw", "raw")          # the value is the kernel's mode (VIAI_UTT_*)
SILENCE_CLASS = 127                                       # utils/audio.py:58 compares with 127 whatever the number of classes
# The shortest waveform the front-end kernels take: every kernel of csrc/audio.hip guards (or range-checks) each sample index and the entry points
# refuse only frames < 1, and lws_num_frames(n) >= 2 for every n >= 1 with hop <= fft.  So one sample; nothing (n = 0) is refused.
MIN_SAMPLES = 1

Utterance = namedtuple("Utterance", "signal mel timesteps start end chunk wav")
Utterance.__doc__ = """One training pair.  signal (N * hop,) int32 classes or fp32; mel (N, num_mels) fp32 contiguous; timesteps = N * hop;
start, end: the trim inside the chunk (end exclusive); chunk: the chunk's index in the file; wav: the trimmed, rescaled waveform (end - start,),
a view of a 16-byte aligned row -- what the mel was computed from."""


def chunk_bounds(n, chunk_samples):
    """librivox.py:56-63: n // chunk_samples chunks as (start, end) pairs, the last one running to the end of the file; none when the file is
    shorter than one chunk."""
    n, chunk_samples = int(n), int(chunk_samples)
    if chunk_samples < 1:
        raise ValueError("chunk_bounds: chunk_samples >= 1")
    k = n // chunk_samples if n > 0 else 0
    return [(i * chunk_samples, n if i == k - 1 else (i + 1) * chunk_samples) for i in range(k)]


def signal_layout(length, fft, hop):
    """(l, r, N, N * hop) for a trimmed signal of `length` samples: the padding of `lws_pad_lr`, the frames of `lws_num_frames` and the length
    the padded signal is cut to (librivox.py:92-102)."""
    length, fft, hop = int(length), int(fft), int(hop)
    if length < 0 or hop < 1 or hop > fft:
        raise ValueError("signal_layout: length >= 0 and 1 <= hop <= fft")
    l, r = lws_pad_lr(length, fft, hop)
    N = lws_num_frames(length, fft, hop)
    return l, r, N, N * hop


def trim_bounds_host(classes, thr, silence_class=SILENCE_CLASS):
    """`start_and_end_indices` (utils/audio.py:56-67) on a CPU integer array, without its asserts: start = the first index whose class is more than
    `thr` away from `silence_class`, else len(classes); end = the last such index among i >= 2, else -1.  The trimmed signal is
    classes[start:end], END EXCLUSIVE.  `viai_utt_trim_bounds` is specified against this function."""
    k = np.asarray(classes.cpu() if isinstance(classes, torch.Tensor) else classes).astype(np.int64).reshape(-1)
    active = np.abs(k - int(silence_class)) > int(thr)
    hit = np.flatnonzero(active)
    start = int(hit[0]) if hit.size else int(k.size)
    hit = hit[hit >= 2]
    end = int(hit[-1]) if hit.size else -1
    return start, end


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _require(wav, what):
    if not isinstance(wav, torch.Tensor) or wav.dim() != 1:
        raise ValueError("%s: wav is an (n,) tensor" % what)
    if not wav.is_cuda:
        raise _lib.ViaiLibraryError("%s runs on the GPU only; no CPU fallback" % what)


def trim_bounds(wav, chunks, silence_threshold=2, mu=255, amax=None, rescaling_max=0.999, silence_class=SILENCE_CLASS, out=None):
    """`viai_utt_trim_bounds`: wav (n,) fp32 on the GPU, chunks a list of (start, end) -> (len(chunks), 2) int32 ON THE DEVICE, (start, end) inside each
    chunk with the sentinels (length, -1).  amax: a one-element fp32 device tensor holding max |wav|, or None for no rescaling.  No synchronisation."""
    _require(wav, "trim_bounds")
    if not chunks:
        raise ValueError("trim_bounds: no chunk")
    lib = _lib.load()
    tab = torch.tensor([[a for a, _ in chunks], [b - a for a, b in chunks]], dtype=torch.int32).to(wav.device)
    bounds = torch.empty(len(chunks), 2, dtype=torch.int32, device=wav.device) if out is None else out
    _lib.check(lib.viai_utt_trim_bounds(wav.data_ptr(), wav.numel(), tab[0].data_ptr(), tab[1].data_ptr(), len(chunks),
                                        0 if amax is None else amax.data_ptr(), float(rescaling_max), int(mu), int(silence_threshold),
                                        int(silence_class), bounds.data_ptr(), _stream()), "viai_utt_trim_bounds")
    return bounds


class UtterancePreprocessor:
    """front: a `MelFrontEnd` (default: one built from `AudioConfig` on the waveform's device at the first call, as `AudioInpainter` builds its own).
    input_type: "mulaw-quantize" (int32 classes, trimmed), "mulaw" or "raw" (floats, not trimmed: librivox.py:76-85).
    silence_threshold: 2, the value of the reference's configuration (tools/oracle_stubs/Config.py).  rescaling / rescaling_max: True / 0.999 are the
    values of the upstream wavenet_vocoder hparams; the reference's stub configuration does not carry them.
    chunk_samples: None = int(8.0 * sample_rate).  skip_silent: drop a chunk without an active sample where the reference asserts."""

    def __init__(self, front=None, input_type="mulaw-quantize", quantize_channels=256, silence_threshold=2, rescaling=True, rescaling_max=0.999,
                 chunk_samples=None, skip_silent=False):
        if input_type not in INPUT_TYPES:
            raise ValueError("UtterancePreprocessor: input_type is one of %s, not %r" % (", ".join(INPUT_TYPES), input_type))
        if int(quantize_channels) < 2:
            raise ValueError("UtterancePreprocessor: quantize_channels >= 2")
        if silence_threshold < 0:
            raise ValueError("UtterancePreprocessor: silence_threshold >= 0")
        cfg = AudioConfig if front is None else front.cfg
        if chunk_samples is None:
            chunk_samples = int(8.0 * cfg.sample_rate)
        if int(chunk_samples) < 1:
            raise ValueError("UtterancePreprocessor: chunk_samples >= 1")
        if cfg.hop_size < 1 or cfg.hop_size > cfg.fft_size:
            raise ValueError("UtterancePreprocessor: 1 <= hop_size <= fft_size")
        self.front, self.cfg = front, cfg
        self.input_type, self.mode = input_type, INPUT_TYPES.index(input_type)
        self.mu = int(quantize_channels) - 1
        self.silence_threshold = int(silence_threshold)
        self.rescaling, self.rescaling_max = bool(rescaling), float(rescaling_max)
        self.chunk_samples = int(chunk_samples)
        self.skip_silent = bool(skip_silent)

    def __call__(self, wav):
        """wav (n,) fp32 on the GPU -> a list of `Utterance`, one per chunk, in chunk order (empty when the file is shorter than one chunk).
        One device-to-host read per file -- the bounds and max |wav|, which size the outputs -- and none for "mulaw" / "raw" without rescaling.
        ValueError: a chunk without an active sample, or whose trim is empty (unless skip_silent); a file of silence with rescaling."""
        _require(wav, "UtterancePreprocessor")
        cfg = self.cfg
        fft, hop = int(cfg.fft_size), int(cfg.hop_size)
        n = wav.numel()
        if n < MIN_SAMPLES:
            raise ValueError("UtterancePreprocessor: the front end needs at least %d sample(s), got %d" % (MIN_SAMPLES, n))
        if n > 2 ** 31 - 1:
            raise ValueError("UtterancePreprocessor: %d samples do not fit the kernels' int32 indices" % n)
        chunks = chunk_bounds(n, self.chunk_samples)
        if not chunks:
            return []
        lib = _lib.load()
        dev = wav.device
        if self.front is None:
            self.front = MelFrontEnd(AudioConfig, device=dev)
        wav = wav.float().contiguous()
        if wav.data_ptr() % 16:
            wav = wav.clone()                                        # viai_absmax reads 16-byte groups
        nc = len(chunks)
        trim = self.mode == 0
        # bounds (nc, 2) and, behind them, the bits of max |wav|: one buffer, one read
        meta = torch.zeros(2 * nc + 1, dtype=torch.int32, device=dev)
        amax = None
        if self.rescaling:
            amax = meta[2 * nc:].view(torch.float32)
            _lib.check(lib.viai_absmax(wav.data_ptr(), n, amax.data_ptr(), _stream()), "viai_absmax")
        if trim:
            trim_bounds(wav, chunks, self.silence_threshold, self.mu, amax, self.rescaling_max, out=meta[:2 * nc].view(nc, 2))
        if trim or self.rescaling:
            host = meta.cpu()                                        # the one synchronisation of the call
            if self.rescaling and float(host[2 * nc:].view(torch.float32)) == 0.0:
                raise ValueError("UtterancePreprocessor: the file is all zeros, nothing to rescale by")
        if trim:
            found = host[:2 * nc].view(nc, 2).tolist()
        else:
            found = [(0, b - a) for a, b in chunks]
        kept = []
        for c, ((a, b), (s, e)) in enumerate(zip(chunks, found)):
            if s >= b - a or e < 0 or e <= s:
                if self.skip_silent:
                    continue
                raise ValueError("UtterancePreprocessor: chunk %d (samples %d to %d) has no sample more than %d classes away from silence "
                                 "(start %d, end %d)" % (c, a, b, self.silence_threshold, s, e))
            kept.append((c, a, b, s, e))
        if not kept:
            return []
        row_off, sig_off, ro, so = [], [], 0, 0
        for _, _, _, s, e in kept:
            row_off.append(ro)
            sig_off.append(so)
            ro += (e - s + 3) // 4 * 4                               # every row and signal starts on a 16-byte boundary
            so += (signal_layout(e - s, fft, hop)[3] + 3) // 4 * 4
        if max(ro, so) > 2 ** 31 - 1:
            raise ValueError("UtterancePreprocessor: the outputs of this file do not fit the kernels' int32 indices")
        nk = len(kept)
        tab = torch.tensor([a for _, a, _, _, _ in kept] + [b - a for _, a, b, _, _ in kept] + [v for k in kept for v in k[3:5]] + row_off + sig_off,
                           dtype=torch.int32).to(dev)
        rows = torch.empty(ro, dtype=torch.float32, device=dev)
        signal = torch.empty(so, dtype=torch.int32 if trim else torch.float32, device=dev)
        _lib.check(lib.viai_utt_pack(wav.data_ptr(), n, tab[0:].data_ptr(), tab[nk:].data_ptr(), tab[2 * nk:].data_ptr(), nk,
                                     max(b - a for _, a, b, _, _ in kept), 0 if amax is None else amax.data_ptr(), self.rescaling_max, self.mode,
                                     self.mu, fft, hop, tab[4 * nk:].data_ptr(), rows.data_ptr(), ro, tab[5 * nk:].data_ptr(), signal.data_ptr(), so,
                                     _stream()), "viai_utt_pack")
        # the mels of all rows in one ragged call, written (N, num_mels); a front end without `ragged` is called once per row as before
        mels = None
        if hasattr(self.front, "ragged"):
            mels = self.front.ragged(rows, [e - s for _, _, _, s, e in kept], row_off, time_major=True)
        out = []
        for i, ((c, _, _, s, e), r0, s0) in enumerate(zip(kept, row_off, sig_off)):
            T = e - s
            _, _, N, steps = signal_layout(T, fft, hop)
            row = rows[r0:r0 + T]
            mel = mels[i] if mels is not None else self.front(row[None])[0, 0].t().contiguous()
            out.append(Utterance(signal[s0:s0 + steps], mel, steps, s, e, c, row))
        return out
