"""How good an inpainted clip is, measured on the device (csrc/metrics.hip).

    wave     SNR and SI-SDR over the regenerated samples                    wave_gap_stats -> snr_db, si_sdr_db
    frames   L1, PSNR and log-spectral distance over selected mel frames    mel_frame_stats -> mel_l1, mel_psnr_db, mel_lsd_db
    image    SSIM of the mel around the selected frames                     mel_ssim
    report   all of them over the damaged region of one `AudioInpainter` call                              inpainting_report

The kernels return fp64 SUMS per stream, taken in a fixed order (no atomics): the same inputs give the same bits, and a clip's row does not depend
on the batch it is in.  The derived figures are plain torch on those rows and are `nan` where nothing was counted.  Regions are the ones the
inpainter already keeps on the device: gap bounds in samples, and the (B, 1, 1, T) time mask (1 = known, 0 = damaged).
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib
from .ops import _stream
from .wavenet_inpaint import _per_stream

WHERE = {"all": 0, "damaged": 1, "clean": 2}
_KIND_WAVE, _KIND_FRAMES, _KIND_SSIM = 0, 1, 2       # VIAI_METRIC_* of include/viai_hip.h
MAX_WIN = 31


def _gpu(what, *tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise _lib.ViaiLibraryError("%s runs on the GPU only; no CPU fallback" % what)


def _workspace(kind, B, a, T, taps, dev):
    n = int(_lib.load().viai_metrics_ws_doubles(kind, B, a, T, taps))
    if n < 1:
        raise ValueError("metrics: no launch geometry for B = %d, %d x %d" % (B, a, T))
    return torch.empty(n, dtype=torch.float64, device=dev)


def _mel_pair(what, ref, est, mask, where):
    """the checks every mel metric shares; returns (B, F, T, where code)"""
    if ref.dim() != 4 or ref.size(1) != 1 or min(ref.shape) < 1:
        raise ValueError("%s: ref is (B, 1, F, T)" % what)
    if est.shape != ref.shape:
        raise ValueError("%s: ref %s and est %s differ in shape" % (what, tuple(ref.shape), tuple(est.shape)))
    if where not in WHERE:
        raise ValueError("%s: where is \"damaged\", \"clean\" or \"all\", not %r" % (what, where))
    B, _, F, T = ref.shape
    if mask is None:
        if where != "all":
            raise ValueError("%s: where=%r needs the (B, 1, 1, T) time mask" % (what, where))
    elif mask.numel() != B * T:
        raise ValueError("%s: mask is (B, 1, 1, T) = (%d, 1, 1, %d)" % (what, B, T))
    return B, F, T, WHERE[where]


def _f32(t):
    return None if t is None else t.float().contiguous()


def _ptr(t):
    return 0 if t is None else t.data_ptr()


# ----------------------------------------------------------------------------------------------------------------------- samples of the gap
def wave_gap_stats(ref, est, gap_start, gap_len):
    """ref, est (B, n) floats on the GPU; gap_start / gap_len in samples, one int, a list or a (B,) tensor, as `AudioInpainter` takes them (a gap
    must lie inside the clip; length 0 = no gap).  Returns the (B, 5) float64 rows {count, sum ref^2, sum est^2, sum (ref - est)^2, sum ref est}
    over [gap_start, gap_start + gap_len) (`viai_wave_gap_stats`)."""
    if ref.dim() != 2 or ref.size(0) < 1 or ref.size(1) < 1:
        raise ValueError("wave_gap_stats: ref is (B, n)")
    if est.shape != ref.shape:
        raise ValueError("wave_gap_stats: ref %s and est %s differ in shape" % (tuple(ref.shape), tuple(est.shape)))
    B, n = ref.shape
    gs, gl = _per_stream(gap_start, B, "gap_start"), _per_stream(gap_len, B, "gap_len")
    if bool((gs < 0).any()) or bool((gl < 0).any()) or bool((gs + gl > n).any()):
        raise ValueError("wave_gap_stats: a gap must lie inside the clip's %d samples" % n)
    _gpu("wave_gap_stats", ref, est)
    ref, est = _f32(ref), _f32(est)
    dev = ref.device
    g0, glen = torch.stack((gs, gl)).to(torch.int32).to(dev)              # one upload for both vectors
    out = torch.empty(B, 5, dtype=torch.float64, device=dev)
    ws = _workspace(_KIND_WAVE, B, n, 0, 0, dev)
    _lib.check(_lib.load().viai_wave_gap_stats(ref.data_ptr(), est.data_ptr(), g0.data_ptr(), glen.data_ptr(), out.data_ptr(), ws.data_ptr(), B, n,
                                               _stream()), "viai_wave_gap_stats")
    return out


def _nan_where_empty(value, count):
    return torch.where(count > 0, value, torch.full_like(value, float("nan")))


def snr_db(stats):
    """10 log10(sum ref^2 / sum err^2) per row of `wave_gap_stats`; nan where count == 0"""
    stats = stats.double()
    return _nan_where_empty(10.0 * torch.log10(stats[:, 1] / stats[:, 3]), stats[:, 0])


def si_sdr_db(stats):
    """Scale-invariant SDR per row of `wave_gap_stats`: with alpha = sum ref est / sum ref^2 the target is alpha ref and the distortion
    est - alpha ref, 10 log10(alpha^2 sum ref^2 / (sum est^2 - 2 alpha sum ref est + alpha^2 sum ref^2)); nan where count == 0"""
    stats = stats.double()
    rr, ee, re = stats[:, 1], stats[:, 2], stats[:, 4]
    alpha = re / rr
    target = alpha * alpha * rr
    return _nan_where_empty(10.0 * torch.log10(target / (ee - 2.0 * alpha * re + target)), stats[:, 0])


# ----------------------------------------------------------------------------------------------------------------------- mel frames
def mel_frame_stats(ref, est, mask=None, where="damaged", min_level_db=-100):
    """ref, est (B, 1, F, T) normalised mels on the GPU, mask (B, 1, 1, T) (1 = known, 0 = damaged) or None; where: "damaged" (mask == 0), "clean"
    (mask != 0) or "all" (the only choice without a mask).  Returns the (B, 4) float64 rows {frames counted, sum |d|, sum d^2,
    sum_t sqrt(mean_f (db_range d)^2)} with d = est - ref and db_range = -min_level_db (`viai_mel_frame_stats`)."""
    B, F, T, code = _mel_pair("mel_frame_stats", ref, est, mask, where)
    _gpu("mel_frame_stats", ref, est, mask)
    ref, est, mask = _f32(ref), _f32(est), _f32(mask)
    out = torch.empty(B, 4, dtype=torch.float64, device=ref.device)
    ws = _workspace(_KIND_FRAMES, B, F, T, 0, ref.device)
    _lib.check(_lib.load().viai_mel_frame_stats(ref.data_ptr(), est.data_ptr(), _ptr(mask), out.data_ptr(), ws.data_ptr(), B, F, T, code,
                                                float(-min_level_db), _stream()), "viai_mel_frame_stats")
    return out


def mel_l1(stats, num_mels):
    """mean |d| over the num_mels x count values of the counted frames, per row of `mel_frame_stats`; nan where no frame is counted"""
    stats = stats.double()
    return _nan_where_empty(stats[:, 1] / (stats[:, 0] * int(num_mels)), stats[:, 0])


def mel_psnr_db(stats, num_mels):
    """10 log10(1 / MSE), peak 1 (the normalised mel's range), per row of `mel_frame_stats`; nan where no frame is counted"""
    stats = stats.double()
    return _nan_where_empty(10.0 * torch.log10(stats[:, 0] * int(num_mels) / stats[:, 2]), stats[:, 0])


def mel_lsd_db(stats):
    """log-spectral distance in dB, the mean over the counted frames of the per-frame RMS dB error; nan where no frame is counted"""
    stats = stats.double()
    return _nan_where_empty(stats[:, 3] / stats[:, 0], stats[:, 0])


# ----------------------------------------------------------------------------------------------------------------------- SSIM
def gaussian_window(win=11, sigma=1.5):
    """the `win` taps of Wang et al.'s window as Python floats (doubles), normalised to sum 1"""
    g = [math.exp(-((i - win // 2) ** 2) / (2.0 * float(sigma) ** 2)) for i in range(win)]
    total = math.fsum(g)
    return [v / total for v in g]


def mel_ssim_stats(ref, est, mask=None, where="damaged", data_range=1.0, win=11, sigma=1.5):
    """(B, 2) float64 rows {window positions counted, sum of ssim} (`viai_mel_ssim`); arguments as `mel_ssim`"""
    B, F, T, code = _mel_pair("mel_ssim", ref, est, mask, where)
    win = int(win)
    if win < 1 or win % 2 == 0 or win > MAX_WIN:
        raise ValueError("mel_ssim: win is odd and at most %d, not %d" % (MAX_WIN, win))
    if F < win or T < win:
        raise ValueError("mel_ssim: a %d x %d mel holds no %d x %d window" % (F, T, win, win))
    if not sigma > 0 or not data_range > 0:
        raise ValueError("mel_ssim: sigma > 0 and data_range > 0")
    _gpu("mel_ssim", ref, est, mask)
    ref, est, mask = _f32(ref), _f32(est), _f32(mask)
    taps = (C.c_double * win)(*gaussian_window(win, sigma))
    out = torch.empty(B, 2, dtype=torch.float64, device=ref.device)
    ws = _workspace(_KIND_SSIM, B, F, T, win, ref.device)
    c1, c2 = (0.01 * float(data_range)) ** 2, (0.03 * float(data_range)) ** 2
    _lib.check(_lib.load().viai_mel_ssim(ref.data_ptr(), est.data_ptr(), _ptr(mask), C.cast(taps, C.c_void_p), out.data_ptr(), ws.data_ptr(), B, F, T,
                                         win, code, c1, c2, _stream()), "viai_mel_ssim")
    return out


def mel_ssim(ref, est, mask=None, where="damaged", data_range=1.0, win=11, sigma=1.5):
    """Mean SSIM per clip, (B,) float64.  Wang et al.'s formula with a separable Gaussian window of `win` taps (odd, <= 31) and population moments,
    c1 = (0.01 data_range)^2, c2 = (0.03 data_range)^2, over the window positions that lie wholly inside the F x T image ("valid" mode) and whose
    CENTRE frame satisfies `where` against the mask.  Frames within win // 2 of the clip's ends are no centre of any position: damage there is not
    seen by this figure; nan where nothing is counted."""
    stats = mel_ssim_stats(ref, est, mask, where, data_range, win, sigma)
    return _nan_where_empty(stats[:, 1] / stats[:, 0], stats[:, 0])


# ----------------------------------------------------------------------------------------------------------------------- one inpainter call
def inpainting_report(inpainter, clean_wav, out_wav, gap_start, gap_len, parts):
    """The figures of one `AudioInpainter` call: out_wav, parts = inpainter(damaged, gap_start, gap_len, return_parts=True), against the clean clip.

    Waveform: SNR and SI-SDR of out_wav against clean_wav over the gap's samples.  Mel: the generator's `parts["fake"]` against the mel of the CLEAN
    clip -- `inpainter.front` on the aligned clean clip, fft - hop zeros in front as the inpainter aligns its input -- over the damaged frames
    (`parts["mask"] == 0`).  Returns a dict of (B,) float64 tensors snr_db, si_sdr_db, mel_l1, mel_psnr_db, mel_lsd_db, mel_ssim, and the counts
    `samples` and `frames`."""
    from .inpaint import wav_align
    cfg = inpainter.front.cfg
    l = int(cfg.fft_size) - int(cfg.hop_size)
    if clean_wav.dim() != 2 or out_wav.shape != clean_wav.shape:
        raise ValueError("inpainting_report: clean_wav and out_wav are (B, n)")
    mask, fake = parts["mask"], parts["fake"]
    wave = wave_gap_stats(clean_wav, out_wav, gap_start, gap_len)
    none = torch.zeros(clean_wav.size(0), dtype=torch.int32, device=clean_wav.device)
    aligned = wav_align(clean_wav, none, none, l)
    clean_mel = inpainter.front(aligned[:, l:])
    frames = mel_frame_stats(clean_mel, fake, mask, "damaged", cfg.min_level_db)
    return {"snr_db": snr_db(wave), "si_sdr_db": si_sdr_db(wave), "mel_l1": mel_l1(frames, fake.size(2)), "mel_psnr_db": mel_psnr_db(frames, fake.size(2)),
            "mel_lsd_db": mel_lsd_db(frames), "mel_ssim": mel_ssim(clean_mel, fake, mask, "damaged"), "samples": wave[:, 0].clone(),
            "frames": frames[:, 0].clone()}
