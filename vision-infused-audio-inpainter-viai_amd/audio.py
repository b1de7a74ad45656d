"""On-device mel front end: host side of `viai_stft_mel` (reference: utils/audio.py:70-144).

`MelFrontEnd(cfg)(wav, mask=None)` == normalised mel spectrograms of a batch of clips, computed by the
fused STFT -> |.| -> mel -> dB -> [0,1] (-> mask) HIP kernel.  The analysis window and mel basis are built
once on the host (numpy) following the lws / librosa conventions the reference relies on; since neither
library is available to check against, this stage is "parity unpinned" (DESIGN.md §4).
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib


class AudioConfig:
    sample_rate = 16000
    fft_size = 1024
    hop_size = 256
    num_mels = 80
    fmin = 125
    fmax = 7600
    min_level_db = -100
    ref_level_db = 20


def lws_num_frames(length, fsize, fshift):
    """utils/audio.py:90-98"""
    pad = fsize - fshift
    return (length + pad * 2 - fsize) // fshift + (1 if length % fshift == 0 else 2)


def lws_pad_lr(length, fsize, fshift):
    """utils/audio.py:101-108"""
    M = lws_num_frames(length, fsize, fshift)
    pad = fsize - fshift
    return pad, pad + (M - 1) * fshift + fsize - (length + 2 * pad)


def sqrt_hann_window(fsize, fshift):
    n = np.arange(fsize, dtype=np.float64)
    return np.sqrt((0.5 - 0.5 * np.cos(2.0 * np.pi * n / (fsize - 1))) * 2.0 * fshift / fsize)


def slaney_mel_basis(sr, n_fft, n_mels, fmin, fmax):
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0

    def hz2mel(f):
        f = np.asarray(f, dtype=np.float64)
        return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, 1e-10) / min_log_hz) / logstep, f / f_sp)

    def mel2hz(m):
        m = np.asarray(m, dtype=np.float64)
        return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)
    freqs = np.linspace(0, sr / 2.0, n_fft // 2 + 1)
    edges = mel2hz(np.linspace(hz2mel(fmin), hz2mel(fmax), n_mels + 2))
    ramps = edges[:, None] - freqs[None, :]
    fd = np.diff(edges)
    w = np.maximum(0, np.minimum(-ramps[:-2] / fd[:-1, None], ramps[2:] / fd[1:, None]))
    return w * (2.0 / (edges[2:n_mels + 2] - edges[:n_mels]))[:, None]


class MelFrontEnd:
    def __init__(self, cfg=AudioConfig, device="cuda"):
        self.cfg = cfg
        self.device = torch.device(device)
        self.window = torch.tensor(sqrt_hann_window(cfg.fft_size, cfg.hop_size), dtype=torch.float32, device=self.device)
        basis = slaney_mel_basis(cfg.sample_rate, cfg.fft_size, cfg.num_mels, cfg.fmin, cfg.fmax)
        self.basis_t = torch.tensor(np.ascontiguousarray(basis.T), dtype=torch.float32, device=self.device)   # [bins][mels]
        # support of every band (the triangles are a few bins wide): what viai_stft_mel_banded reads instead of all fft/2 + 1 bins
        nz = basis.astype(np.float32) != 0
        lo = np.where(nz.any(1), nz.argmax(1), 0)
        hi = np.where(nz.any(1), nz.shape[1] - nz[:, ::-1].argmax(1), 0)
        self.band_lo = torch.tensor(lo, dtype=torch.int32, device=self.device)
        self.band_cnt = torch.tensor(hi - lo, dtype=torch.int32, device=self.device)

    def num_frames(self, n_samples):
        return lws_num_frames(n_samples, self.cfg.fft_size, self.cfg.hop_size)

    def __call__(self, wav: torch.Tensor, mask: torch.Tensor = None) -> torch.Tensor:
        """wav (B, n_samples) fp32 on the GPU -> (B, 1, num_mels, frames); mask (B, frames) optional."""
        lib = _lib.load()
        if not wav.is_cuda:
            raise _lib.ViaiLibraryError("MelFrontEnd runs on the GPU only; no CPU fallback")
        wav = wav.contiguous().float()
        B, n = wav.shape
        frames = self.num_frames(n)
        c = self.cfg
        out = torch.empty((B, 1, c.num_mels, frames), device=wav.device, dtype=torch.float32)
        m = None
        if mask is not None:
            m = mask.reshape(B, frames).contiguous().float()
        st = torch.cuda.current_stream().cuda_stream
        if c.fft_size == 1024 and not getattr(self, "force_dense", False):
            _lib.check(lib.viai_stft_mel_banded(wav.data_ptr(), self.window.data_ptr(), self.basis_t.data_ptr(), self.band_lo.data_ptr(),
                                                self.band_cnt.data_ptr(), 0 if m is None else m.data_ptr(), out.data_ptr(), B, n, c.fft_size,
                                                c.hop_size, c.num_mels, frames, float(c.min_level_db), float(c.ref_level_db), st),
                       "viai_stft_mel_banded")
        else:
            _lib.check(lib.viai_stft_mel(wav.data_ptr(), self.window.data_ptr(), self.basis_t.data_ptr(),
                                         0 if m is None else m.data_ptr(), out.data_ptr(), B, n, c.fft_size, c.hop_size,
                                         c.num_mels, frames, float(c.min_level_db), float(c.ref_level_db), st), "viai_stft_mel")
        return out

    def ragged(self, wav, lengths=None, offsets=None, mask=None, time_major=False):
        """Mel of clips of DIFFERENT lengths in one call (`viai_stft_mel_ragged`, table layout in include/viai_hip.h).

        wav: a 1-D fp32 GPU tensor holding the rows, with `lengths` (host ints, >= 1 each) and optionally `offsets` (host ints, in samples; default:
        the rows packed back to back) -- rows must lie inside `wav`, may leave gaps and may overlap; or a list of 1-D GPU tensors, which this method
        packs into one buffer at offsets that are multiples of 4 samples, so that even-length rows take the r512 route.
        mask: optional, flat, one float per output frame of all rows in row order (sum of the rows' frame counts).
        -> a list of per-row tensors, views of ONE allocation, each contiguous: (num_mels, frames_r), or (frames_r, num_mels) with time_major.

        Row r gets the bits of `self(row_r[None])[0, 0]` on a row whose first sample is aligned as this one's is (8-byte aligned or not: the kernel
        family is chosen per row by length and alignment, as `viai_stft_mel_route` reports): for rows at even offsets of an aligned buffer, and for a
        list of tensors, that is the result on a fresh copy of the row.  No device-to-host read; one table upload and one C call.
        For fft_size != 1024, where only the dense one-frame-per-block kernel exists, and with `force_dense`, the method loops over the rows with
        `__call__` and copies each result into the shared allocation."""
        c = self.cfg
        fft, hop, n_mels = int(c.fft_size), int(c.hop_size), int(c.num_mels)
        if hop < 1 or hop > fft or n_mels < 1:
            raise ValueError("MelFrontEnd.ragged: 1 <= hop_size <= fft_size and num_mels >= 1")
        packed = isinstance(wav, (list, tuple))
        if packed:
            if lengths is not None or offsets is not None:
                raise ValueError("MelFrontEnd.ragged: a list of rows carries its own lengths; lengths / offsets go with a 1-D buffer")
            if len(wav) == 0:
                raise ValueError("MelFrontEnd.ragged: no row")
            if any(not isinstance(t, torch.Tensor) or t.dim() != 1 for t in wav):
                raise ValueError("MelFrontEnd.ragged: every row is an (n,) tensor")
            lengths = [int(t.numel()) for t in wav]
            offsets, o = [], 0
            for n in lengths:
                offsets.append(o)
                o += (n + 3) // 4 * 4
            span = o
            tensors = list(wav)
        else:
            if not isinstance(wav, torch.Tensor) or wav.dim() != 1:
                raise ValueError("MelFrontEnd.ragged: wav is an (n,) tensor or a list of them")
            if lengths is None:
                raise ValueError("MelFrontEnd.ragged: a 1-D buffer needs the rows' lengths")
            lengths = [int(n) for n in lengths]
            if len(lengths) == 0:
                raise ValueError("MelFrontEnd.ragged: no row")
            if offsets is None:
                offsets, o = [], 0
                for n in lengths:
                    offsets.append(o)
                    o += n
            offsets = [int(o) for o in offsets]
            if len(offsets) != len(lengths):
                raise ValueError("MelFrontEnd.ragged: %d lengths but %d offsets" % (len(lengths), len(offsets)))
            span = int(wav.numel())
            tensors = [wav]
        for r, (o, n) in enumerate(zip(offsets, lengths)):
            if n < 1:
                raise ValueError("MelFrontEnd.ragged: row %d has length %d; the front end needs at least one sample" % (r, n))
            if n > 2 ** 29 - 1:
                raise ValueError("MelFrontEnd.ragged: row %d has %d samples, more than the kernels' 2^29 - 1" % (r, n))
            if o < 0 or o + n > span:
                raise ValueError("MelFrontEnd.ragged: row %d (samples %d to %d) does not lie inside the %d samples of wav" % (r, o, o + n, span))
        nr = len(lengths)
        frames = [lws_num_frames(n, fft, hop) for n in lengths]
        total = sum(frames)
        if total > 2 ** 31 - 1:
            raise ValueError("MelFrontEnd.ragged: %d frames do not fit the kernels' int32 indices" % total)
        if mask is not None and (not isinstance(mask, torch.Tensor) or mask.numel() != total):
            raise ValueError("MelFrontEnd.ragged: mask holds one value per output frame (%d)" % total)
        if any(not t.is_cuda for t in tensors) or (mask is not None and not mask.is_cuda):
            raise _lib.ViaiLibraryError("MelFrontEnd runs on the GPU only; no CPU fallback")
        lib = _lib.load()
        dev = tensors[0].device
        if packed:
            buf = torch.zeros(span, dtype=torch.float32, device=dev)
            for t, o, n in zip(tensors, offsets, lengths):
                buf[o:o + n].copy_(t)
        else:
            buf = wav.contiguous().float()
        m = None if mask is None else mask.reshape(-1).contiguous().float()
        out = torch.empty(n_mels * total, dtype=torch.float32, device=dev)
        fo = np.concatenate([[0], np.cumsum(frames)]).astype(np.int64)
        shape = (lambda f: (f, n_mels)) if time_major else (lambda f: (n_mels, f))
        views = [out[n_mels * int(fo[r]):n_mels * int(fo[r + 1])].view(shape(frames[r])) for r in range(nr)]
        if fft != 1024 or getattr(self, "force_dense", False):
            for r in range(nr):
                one = self(buf[offsets[r]:offsets[r] + lengths[r]][None], None if m is None else m[int(fo[r]):int(fo[r + 1])][None])[0, 0]
                views[r].copy_(one.t() if time_major else one)
            return views
        # the tables, one int32 host buffer: row_off (int64) | row_len | row_frames | frame_off | items
        head = np.empty(5 * nr + 1, dtype=np.int32)
        head[:2 * nr].view(np.int64)[:] = offsets
        head[2 * nr:3 * nr] = lengths
        fam_items = np.zeros(3, dtype=np.int32)
        al = int(buf.data_ptr() % 8 == 0)

        def plan(tab, n_items):
            p = tab.ctypes.data
            return lib.viai_stft_mel_ragged_plan(p, p + 8 * nr, nr, fft, hop, n_mels, al, p + 12 * nr, p + 16 * nr, None,
                                                 p + 4 * (5 * nr + 1) if n_items else None, n_items, fam_items.ctypes.data)
        need = plan(head, 0)
        if need < 1:
            raise ValueError("MelFrontEnd.ragged: viai_stft_mel_ragged_plan refuses these rows at fft %d, hop %d, %d bands" % (fft, hop, n_mels))
        tab = np.empty(5 * nr + 1 + 2 * need, dtype=np.int32)
        tab[:3 * nr] = head[:3 * nr]
        if plan(tab, need) != 0 or tab[3 * nr:4 * nr].tolist() != frames:
            raise _lib.ViaiLibraryError("viai_stft_mel_ragged_plan disagrees with lws_num_frames")
        d = torch.from_numpy(tab).to(dev)
        p = d.data_ptr()
        _lib.check(lib.viai_stft_mel_ragged(buf.data_ptr(), p, p + 8 * nr, p + 12 * nr, p + 16 * nr, p + 4 * (5 * nr + 1), fam_items.ctypes.data, nr,
                                            self.window.data_ptr(), self.basis_t.data_ptr(), self.band_lo.data_ptr(), self.band_cnt.data_ptr(),
                                            0 if m is None else m.data_ptr(), out.data_ptr(), fft, hop, n_mels, int(bool(time_major)),
                                            float(c.min_level_db), float(c.ref_level_db), torch.cuda.current_stream().cuda_stream),
                   "viai_stft_mel_ragged")
        return views


def inv_mel_amplitude(S, min_level_db=None):
    """`_db_to_amp(_denormalize(S))` of utils/audio.py:135-144 in one pass: the normalised mel the generator emits
    -> linear amplitudes (the step after the path; the vocoder consumes the normalised mel directly)."""
    from .ops import _require, _stream
    _require(S)
    S = S if S.is_contiguous() else S.contiguous()
    out = torch.empty_like(S)
    db = float(AudioConfig.min_level_db if min_level_db is None else min_level_db)
    _lib.check(_lib.load().viai_mel_denorm_amp(S.data_ptr(), out.data_ptr(), S.numel(), db, _stream()), "viai_mel_denorm_amp")
    return out
