"""GPU: every kernel and launch branch of the STFT -> mel front end (csrc/audio.hip) against the fp64 numpy oracle, through the C ABI.

tests/test_audio_gpu.py reaches the r512 and the tiled wave kernel on Slaney bases with weights in LDS, one tile group per block, a symmetric
window and nothing on either clip.  Here the window, the basis, its band supports and the two levels are chosen by the test:

  a. bin probe      a one-hot basis makes every output ONE magnitude bin; the output is inverted back to linear amplitude and compared frame by
                    frame in units of that frame's largest magnitude (fp32 FFT error is relative to the frame's energy, not to a weak bin's own
                    value), with min_level_db = -160 and ref_level_db = 40 so that nothing compared is clipped.  All 513 bins on r512, both
                    forms of the wave kernel (reached by each of its three conditions) and the dense kernel; an ASYMMETRIC window (a reversed
                    read would pass under sqrt-Hann); a burst case in which every frame that sees only zeros -- the partner of a burst frame in
                    the two-frames-per-FFT split included -- must be bitwise 0.0.
  b. calibration    no bound is typed in from a GPU run: the same quantity is computed by a plain fp32 pipeline on the CPU (torch.fft.rfft of the
                    fp32 windowed frames, fp32 magnitude, fp32 basis product, fp32 log10) on the same inputs, its worst error against the fp64
                    oracle is the scale, and the kernel may err by MARGIN = 8 times that (sincospif twiddles and radix orders other than
                    pocketfft's; log10f / exp10f / v_log_f32 on the device are not correctly rounded).
  c. real bases     Slaney 80 / 256, the banded kernel (1025 bands), weights read from global memory (sum of band_cnt above 1024 on r512, above
                    2048 on the wave kernel), a fully dense basis, the dense kernel at fft 512 and 2048 with n_mels = 300, hops 256 / 200 / 1024
                    / 255: normalised scale, bound min(2e-4, calibrated as in b).
  d. persistent     more than 256 tile groups on both persistent kernels: a block walks two groups, crosses from one clip into the next, ends on
                    a 5-frame tile, trailing blocks idle.
  e. clips, mask    exact 0.0 below the floor (a silenced span) and exact 1.0 above the ceiling on every route; a non-binary mask is a bitwise
                    fp32 product on every route, the partially filled last tile included.

Every test asserts the kernel family (viai_stft_mel_route) before it launches.  The output buffer is pre-filled with NaN: an element no kernel
wrote fails every comparison.

An all-zero frame has no magnitude to be relative to: the bin probe at an odd n_samples has one (its last frame holds a single sample under
window[0] = 0), the reference is on the floor there, and the kernel must give bitwise 0.0; every other frame must be unclipped in the reference.

Measured on the MI355X (the test prints every figure before it asserts): calibrated tol of the bin probe 1.4e-6 to 1.3e-5 of a frame's largest magnitude
(8 x an fp32 restatement of 1.8e-7 to 1.6e-6, most of it the fp32 rounding of the [0,1] output over 160 dB); kernel worst, as a fraction of tol: r512 0.10 -
0.16, wave 0.10 - 0.16, banded 0.11 - 0.15, dense 0.12 - 0.16.  Normalised scale: calibrated bound 6.4e-7 to 2.3e-5 (never the 2e-4 cap), kernel worst
0.05 - 0.44 of it on every route (0.44: banded at hop 255).
FOUND BY THIS FILE: at hops 254, 255 and 257 the wave kernel was off by up to 9.4e-2 of a frame's largest magnitude in the frames that cross the clip's
start (hops 192, 200, 256, 1024: 1.5e-6); stft_route (csrc/audio.hip) now sends hops that are no multiple of 8 to the frame-batched kernel, and the hop-255
cases here assert that family.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import audio_oracle as A

MARGIN = 8.0
EPS32 = 2.0 ** -23
BINS = 513
R5_WCAP, WAVE_WCAP = 1024, 2048            # weights held in LDS up to these sums of band_cnt (csrc/audio.hip)


# --------------------------------------------------------------------------------------------------------------- inputs
def make_cfg(fft, hop, n_mels, min_db, ref_db):
    class Cfg(A.AudioConfig):
        fft_size, hop_size, num_mels, min_level_db, ref_level_db = fft, hop, n_mels, min_db, ref_db
    return Cfg


def band_support(basis32):
    """[band_lo, band_cnt] of an fp32 basis [n_mels][bins], as viai_amd.audio.MelFrontEnd.__init__ derives them"""
    nz = basis32 != 0
    lo = np.where(nz.any(1), nz.argmax(1), 0)
    hi = np.where(nz.any(1), nz.shape[1] - nz[:, ::-1].argmax(1), 0)
    return lo.astype(np.int32), (hi - lo).astype(np.int32)


@functools.lru_cache(maxsize=None)
def window32(fft, hop, asym=True):
    from viai_amd import synth
    w = A.lws_window(fft, hop)
    if asym:
        w = w * (1.0 + 0.5 * synth.uniform("routes.win", (fft,)).numpy().astype(np.float64))
    return w.astype(np.float32)


def one_hot(n_mels, k0, bins=BINS):
    b = np.zeros((n_mels, bins), np.float32)
    b[np.arange(n_mels), (k0 + np.arange(n_mels)) % bins] = 1.0
    return b


def slaney(n_mels, fft=1024):
    return A.mel_basis(16000, fft, n_mels, 125, 7600).astype(np.float32)


def band_basis(n_mels, width, tag, bins=BINS, scale=0.02):
    """bands of `width` bins (an int, or one per band) at increasing lo with fixed pseudo-random positive weights"""
    from viai_amd import synth
    widths = np.broadcast_to(np.asarray(width), (n_mels,))
    u = synth.uniform(tag, (n_mels, bins), 0.25, 1.0).numpy()
    b = np.zeros((n_mels, bins), np.float32)
    for m in range(n_mels):
        lo = (m * (bins - int(widths.max()))) // max(n_mels - 1, 1)
        b[m, lo:lo + int(widths[m])] = u[m, :int(widths[m])] * np.float32(scale)
    return b


def make_waveform(B, n, tag="routes.wav"):
    from viai_amd import synth
    return synth.waveform(B, n, tag=tag).numpy()


# --------------------------------------------------------------------------------------------------------------- the two CPU pipelines
def ref64(wav, win, basis, fft, hop, min_db, ref_db):
    """fp64 oracle on the fp32 inputs -> (normalised [B][n_mels][frames], |X| [B][frames][bins], unclamped dB [B][n_mels][frames])"""
    cfg = make_cfg(fft, hop, basis.shape[0], min_db, ref_db)
    w64, b64 = win.astype(np.float64), basis.astype(np.float64)
    nrm, mag, raw = [], [], []
    for y in wav:
        y64 = y.astype(np.float64)
        nrm.append(A.melspectrogram(y64, cfg, window=w64, basis=b64))
        mag.append(np.abs(A.stft_lws(y64, fft, hop, w64)))
        with np.errstate(divide="ignore"):
            raw.append(20.0 * np.log10(b64 @ mag[-1].T) - ref_db)
    return np.stack(nrm), np.stack(mag), np.stack(raw)


def pipe32(wav, win, basis, fft, hop, min_db, ref_db):
    """the same stage in plain fp32 on the CPU (the yardstick of the calibration, never the kernel): normalised [B][n_mels][frames] fp32"""
    B, n = wav.shape
    M = A.lws_num_frames(n, fft, hop)
    l, r = A.lws_pad_lr(n, fft, hop)
    yp = torch.nn.functional.pad(torch.from_numpy(np.array(wav, np.float32)), (l, max(r, 0)))
    fr = yp.unfold(1, fft, hop)[:, :M] * torch.from_numpy(win)[None, None, :]
    mag = torch.fft.rfft(fr, dim=2).abs()                                               # [B][M][bins] fp32
    assert mag.dtype == torch.float32
    mel = torch.matmul(torch.from_numpy(basis)[None], mag.transpose(1, 2))
    min_level = torch.tensor(10.0 ** (min_db / 20.0), dtype=torch.float32)
    S = 20.0 * torch.log10(torch.maximum(min_level, mel)) - np.float32(ref_db)
    return ((S - np.float32(min_db)) / np.float32(-min_db)).clamp(0.0, 1.0).numpy()


def to_amp(nrm, min_db, ref_db):
    return 10.0 ** ((np.asarray(nrm, np.float64) * (-min_db) + min_db + ref_db) / 20.0)


# --------------------------------------------------------------------------------------------------------------- the launch
def route(n, fft, hop, n_mels, aligned=True):
    import ctypes as C
    from viai_amd import _lib
    buf = C.create_string_buffer(16)
    ok = _lib.load().viai_stft_mel_route(n, fft, hop, n_mels, int(aligned), buf, 16)
    assert ok == (buf.value != b"")
    return buf.value.decode()


def launch(wav, win, basis, hop, min_db, ref_db, family, fft=1024, mask=None, misalign=False):
    """one call of the C ABI on the kernel family named: 'r512' / 'wave' / 'banded' through viai_stft_mel_banded (asserted with the route
    query BEFORE the launch), 'dense' through viai_stft_mel, whose one kernel serves every fft.  misalign: the clips start one float past an
    8-byte boundary (a view of a larger buffer; .contiguous() would re-align it).  -> [B][n_mels][frames] fp32, NaN where nothing was written"""
    from viai_amd import _lib
    lib = _lib.load()
    B, n = wav.shape
    n_mels = basis.shape[0]
    assert basis.shape[1] == fft // 2 + 1 and win.shape == (fft,) and wav.dtype == np.float32
    frames = A.lws_num_frames(n, fft, hop)
    flat = torch.zeros(B * n + 2, dtype=torch.float32, device="cuda")
    off = 1 if misalign else 0
    x = flat[off:off + B * n].view(B, n)
    x.copy_(torch.from_numpy(np.array(wav, np.float32)))
    assert x.is_contiguous() and (x.data_ptr() & 7) == (4 if misalign else 0)
    d_win = torch.from_numpy(win).cuda()
    d_bt = torch.from_numpy(np.ascontiguousarray(basis.T)).cuda()
    d_mask = None if mask is None else torch.from_numpy(np.ascontiguousarray(mask, np.float32)).cuda()
    out = torch.full((B, n_mels, frames), float("nan"), dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    pm = 0 if d_mask is None else d_mask.data_ptr()
    if family == "dense":
        if fft != 1024:
            assert route(n, fft, hop, n_mels) == "dense"
        err = lib.viai_stft_mel(x.data_ptr(), d_win.data_ptr(), d_bt.data_ptr(), pm, out.data_ptr(), B, n, fft, hop, n_mels, frames,
                                float(min_db), float(ref_db), st)
    else:
        got = route(n, fft, hop, n_mels, not misalign)
        assert got == family, "shape (%d, %d, %d, %d, aligned %d) runs on %r, the test wants %r" % (n, fft, hop, n_mels, not misalign, got, family)
        lo, cnt = band_support(basis)
        total = int(cnt.sum())
        if family == "r512":
            print("  band weights: sum %d -> %s" % (total, "LDS" if total <= R5_WCAP else "global"))
        elif family == "wave":
            print("  band weights: sum %d -> %s" % (total, "LDS" if total <= WAVE_WCAP else "global"))
        d_lo, d_cnt = torch.from_numpy(lo).cuda(), torch.from_numpy(cnt).cuda()
        err = lib.viai_stft_mel_banded(x.data_ptr(), d_win.data_ptr(), d_bt.data_ptr(), d_lo.data_ptr(), d_cnt.data_ptr(), pm, out.data_ptr(),
                                       B, n, fft, hop, n_mels, frames, float(min_db), float(ref_db), st)
    assert err == 0, "hipError_t %d" % err
    torch.cuda.synchronize()
    return out.cpu().numpy()


def zero_bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32) == 0


# --------------------------------------------------------------------------------------------------------------- a. bin probe
P_MIN, P_REF = -160.0, 40.0          # the clips sit at amplitudes 1e-6 and 100


def frame_rel_err(nrm, ref_nrm, mag, min_db, ref_db, live, paired=False):
    """worst over the live frames of max_m |a - a_ref| / max_k |X_ref[frame, k]| -> (worst, [B][frames] per-frame figures).
    paired: the wave and the banded kernel carry frames 2q and 2q + 1 as the real and the imaginary part of ONE complex FFT and separate the two spectra
    afterwards, so the rounding error of either is relative to the energy of both: the scale of a frame is the larger of the pair's two maxima (measured:
    the last frame at hop 255 holds 24 samples under the window's first taps next to a full partner and sits at 9 x the fp32 restatement of its own
    magnitude on the banded kernel, every other frame at 1 x; a leak of the partner's spectrum is still held to MARGIN x 1e-6 of the partner)"""
    d = np.abs(to_amp(nrm, min_db, ref_db) - to_amp(ref_nrm, min_db, ref_db)).max(1)                # [B][frames]
    top = mag.max(2)
    if paired:
        F = top.shape[1]
        partner = np.minimum(np.arange(F) ^ 1, F - 1)                                                # (an odd frame count: the last frame rides alone)
        top = np.maximum(top, top[:, partner])
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(live, d / top, 0.0)
    return float(np.nanmax(e)) if np.isfinite(e).all() else float("inf"), e


def probe_check(name, family, wav, win, basis, hop, misalign=False, min_db=P_MIN, ref_db=P_REF, expect_dead=None):
    ref_nrm, mag, raw = ref64(wav, win, basis, 1024, hop, min_db, ref_db)
    # frames whose windowed samples are all zero have nothing to be relative to: the reference is on the floor, the kernel must give 0.0
    live = mag.max(2) > 0
    if expect_dead is not None:
        assert int((~live).sum()) == expect_dead, (name, int((~live).sum()))
    lv = np.broadcast_to(live[:, None, :], ref_nrm.shape)
    assert np.all((ref_nrm[lv] > 0.0) & (ref_nrm[lv] < 1.0)), "%s: %d compared reference elements are clipped (cap: zero)" % (
        name, int(((ref_nrm[lv] <= 0) | (ref_nrm[lv] >= 1)).sum()))
    assert np.all(ref_nrm[~lv] == 0.0)
    paired = family in ("wave", "banded")
    cal, _ = frame_rel_err(pipe32(wav, win, basis, 1024, hop, min_db, ref_db), ref_nrm, mag, min_db, ref_db, live, paired)
    tol = MARGIN * cal
    got = launch(wav, win, basis, hop, min_db, ref_db, family, misalign=misalign)
    worst, e = frame_rel_err(got, ref_nrm, mag, min_db, ref_db, live, paired)
    b, f = np.unravel_index(np.argmax(e), e.shape)
    print("probe %-26s family %-6s fp32 restatement %.3e  tol %.3e  kernel worst %.3e (clip %d frame %d)  ratio to tol %.2f" % (
        name, family, cal, tol, worst, b, f, worst / tol))
    assert np.all(zero_bits(got[~lv])), "%s: %d elements of all-zero frames are not bitwise 0.0" % (name, int((~zero_bits(got[~lv])).sum()))
    assert worst <= tol, (name, worst, tol, "worst per-frame figures", np.sort(e.reshape(-1))[-4:])
    return got, live


PROBES = {  # name: (family, n_samples, hop, n_mels, k0, asymmetric window, misaligned pointer)
    "r512-k0":            ("r512", 5120, 256, 256, 0, True, False),
    "r512-k256":          ("r512", 5120, 256, 256, 256, True, False),
    "r512-k257":          ("r512", 5120, 256, 256, 257, True, False),
    "r512-k0-sqrt-hann":  ("r512", 5120, 256, 256, 0, False, False),
    "wave-untiled-513":   ("wave", 5120, 256, 513, 0, True, False),
    "wave-untiled-odd-n": ("wave", 5121, 256, 513, 0, True, False),
    "wave-tiled-odd-n":   ("wave", 5121, 256, 256, 257, True, False),
    "hop255-k257":        ("banded", 5120, 255, 256, 257, True, False),       # (the wave kernels take multiples of 8 only: see hop255 below)
    "hop255-513":         ("banded", 5120, 255, 513, 0, True, False),
    "wave-hop200-odd-n":  ("wave", 5121, 200, 513, 0, True, False),           # frames start on multiples of 8 samples, not of 64
    "r512-hop200-k0":     ("r512", 5120, 200, 256, 0, True, False),
    "wave-tiled-offset":  ("wave", 5120, 256, 256, 257, True, True),
    "dense-513":          ("dense", 5120, 256, 513, 0, True, False),
    "dense-513-odd-n":    ("dense", 5121, 256, 513, 0, True, False),
}


@pytest.mark.parametrize("name", list(PROBES))
def test_bin_probe(name):
    family, n, hop, n_mels, k0, asym, mis = PROBES[name]
    wav = make_waveform(2, n)
    frames = A.lws_num_frames(n, 1024, hop)
    assert frames == {(5120, 256): 23, (5121, 256): 24, (5120, 255): 24, (5120, 200): 30, (5121, 200): 30}[(n, hop)]
    # an odd n_samples at hop 256 ends on a frame that holds one sample under window[0] = 0: all zero, one per clip
    probe_check(name, family, wav, window32(1024, hop, asym), one_hot(n_mels, k0), hop, misalign=mis, expect_dead=2 if (n, hop) == (5121, 256) else 0)


def burst_waveform():
    from viai_amd import synth
    w = np.zeros((2, 5120), np.float32)
    u = synth.uniform("routes.burst", (2, 256), -0.2, 0.2).numpy()
    w[0, 1100:1356] = u[0]                  # neither burst starts on a hop: the first and the last frame that see it hold 180 / 76 and 160 / 96 samples of it
    w[1, 2400:2656] = u[1]
    return w


@pytest.mark.parametrize("family", ["r512", "wave", "banded", "dense"])
def test_frame_pair_leak(family):
    """one 256-sample burst per clip at the project's own -100 / 20 levels: the five frames that see it match the oracle in linear amplitude, every
    other frame -- the burst frames' partners in the two-frames-per-FFT split of the wave and banded kernels included -- is bitwise 0.0"""
    wav = burst_waveform()
    n_mels = {"r512": 256, "wave": 513, "banded": 1025, "dense": 513}[family]
    basis = one_hot(n_mels, 0)                              # (1025 bands: the bins twice over, less one)
    win = window32(1024, 256, True)
    mag = np.abs(np.stack([A.stft_lws(y.astype(np.float64), 1024, 256, win.astype(np.float64)) for y in wav]))
    live = mag.max(2) > 0
    for b, first in ((0, 4), (1, 9)):
        seen = np.flatnonzero(live[b])
        assert list(seen) == list(range(first, first + 5)), seen                 # odd- and even-indexed frames, and a partner either side
        assert (seen % 2 == 0).sum() >= 1 and (seen % 2 == 1).sum() >= 1
    probe_check("burst-" + family, family, wav, win, basis, 256, min_db=-100.0, ref_db=20.0, expect_dead=2 * 23 - 10)


# --------------------------------------------------------------------------------------------------------------- c. real bases
def norm_check(name, family, wav, win, basis, hop, fft=1024, misalign=False, min_db=-100.0, ref_db=20.0, ref=None):
    """normalised scale against the oracle: bound min(2e-4, MARGIN x the fp32 restatement's worst error, floored at 2 ulp of 1.0)"""
    ref_nrm = ref64(wav, win, basis, fft, hop, min_db, ref_db)[0] if ref is None else ref[0]
    cal = float(np.abs(pipe32(wav, win, basis, fft, hop, min_db, ref_db).astype(np.float64) - ref_nrm).max()) if ref is None else ref[1]
    bound = min(2e-4, max(MARGIN * cal, 2.0 * EPS32))
    got = launch(wav, win, basis, hop, min_db, ref_db, family, fft=fft, misalign=misalign)
    err = np.abs(got.astype(np.float64) - ref_nrm)
    worst = float(np.nanmax(err)) if not np.isnan(err).any() else float("inf")
    print("normalised %-22s family %-6s fp32 restatement %.3e  bound %.3e  kernel worst %.3e at %s  ratio %.2f" % (
        name, family, cal, bound, worst, np.unravel_index(np.nanargmax(err), err.shape), worst / bound))
    assert worst <= bound, (name, worst, bound)
    return got


def _wl_false_r512():
    b = band_basis(64, 20, "routes.wl.r512")
    assert int(band_support(b)[1].sum()) == 1280 > R5_WCAP
    return b


def _wl_false_wave():
    b = band_basis(128, 20, "routes.wl.wave")
    assert int(band_support(b)[1].sum()) == 2560 > WAVE_WCAP
    return b


def _banded_1025():
    b = band_basis(1025, 1 + np.arange(1025) % 3, "routes.banded", scale=0.1)
    lo, cnt = band_support(b)
    assert cnt.min() == 1 and cnt.max() == 3 and np.all(np.diff(lo) >= 0)
    return b


def _dense_8():
    b = band_basis(8, BINS, "routes.dense8", scale=0.002)
    lo, cnt = band_support(b)
    assert np.all(lo == 0) and np.all(cnt == BINS)
    return b


def _slaney_lds(n_mels):
    b = slaney(n_mels)
    assert int(band_support(b)[1].sum()) <= R5_WCAP                   # weights in LDS on both kernels, as the product runs
    return b


REAL = {  # name: (family, n_samples, fft, hop, basis, misaligned pointer)
    "slaney80-r512":     ("r512", 5120, 1024, 256, lambda: _slaney_lds(80), False),
    "slaney256-r512":    ("r512", 5120, 1024, 256, lambda: _slaney_lds(256), False),
    "slaney80-wave":     ("wave", 5121, 1024, 256, lambda: _slaney_lds(80), False),
    "slaney256-wave":    ("wave", 5120, 1024, 256, lambda: _slaney_lds(256), True),
    "banded-1025":       ("banded", 5120, 1024, 256, _banded_1025, False),
    "banded-1025-odd-n": ("banded", 5121, 1024, 256, _banded_1025, False),     # 24 frames: the 16-byte stores; 23: the scalar ones
    "wl-global-r512":    ("r512", 5120, 1024, 256, _wl_false_r512, False),
    "wl-global-wave":    ("wave", 5121, 1024, 256, _wl_false_wave, False),
    "dense-basis-r512":  ("r512", 5120, 1024, 256, _dense_8, False),
    "dense-basis-wave":  ("wave", 5121, 1024, 256, _dense_8, False),
    "dense-fft512":      ("dense", 5120, 512, 128, lambda: band_basis(300, 9, "routes.d512", bins=257), False),
    "dense-fft2048":     ("dense", 5120, 2048, 512, lambda: band_basis(300, 30, "routes.d2048", bins=1025), False),
    "dense-fft1024-300": ("dense", 5120, 1024, 256, lambda: band_basis(300, 15, "routes.d1024"), False),
    "hop200-r512":       ("r512", 5120, 1024, 200, lambda: _slaney_lds(80), False),
    "hop1024-r512":      ("r512", 5120, 1024, 1024, lambda: _slaney_lds(80), False),
    "hop255":            ("banded", 5120, 1024, 255, lambda: _slaney_lds(80), False),
    "hop254":            ("banded", 5120, 1024, 254, lambda: _slaney_lds(80), False),
    "hop200-wave":       ("wave", 5121, 1024, 200, lambda: _slaney_lds(80), False),
}


@pytest.mark.parametrize("name", list(REAL))
def test_real_basis(name):
    family, n, fft, hop, basis, mis = REAL[name]
    norm_check(name, family, make_waveform(2, n), window32(fft, hop, True), basis(), hop, fft=fft, misalign=mis)


# --------------------------------------------------------------------------------------------------------------- d. persistent loop
LOOPS = {"many-short": (300, 7424, 32, 300), "few-long": (9, 238080, 933, 270)}      # B, n_samples, frames, 32-frame groups


@functools.lru_cache(maxsize=None)
def loop_case(name):
    B, n, frames, groups = LOOPS[name]
    assert A.lws_num_frames(n, 1024, 256) == frames and B * ((frames + 31) // 32) == groups > 256         # both launchers cap the grid at 256 blocks
    wav = make_waveform(B, n, tag="routes.loop." + name)
    win, basis = window32(1024, 256, True), _slaney_lds(80)
    ref_nrm = ref64(wav, win, basis, 1024, 256, -100.0, 20.0)[0]
    cal = float(np.abs(pipe32(wav, win, basis, 1024, 256, -100.0, 20.0).astype(np.float64) - ref_nrm).max())
    for a in (wav, ref_nrm):
        a.setflags(write=False)
    return wav, win, basis, (ref_nrm, cal)


@pytest.mark.parametrize("family", ["r512", "wave"])
@pytest.mark.parametrize("name", list(LOOPS))
def test_persistent_loop(name, family):
    """more tile groups than blocks: per = 2 groups per block (many-short: the trailing blocks idle; few-long: 30 groups per clip, so a block's
    range crosses clips, and the last tile of every clip has 5 of 32 frames).  The wave kernel sees the same data one float off alignment"""
    wav, win, basis, ref = loop_case(name)
    norm_check("loop-%s-%s" % (name, family), family, wav, win, basis, 256, misalign=family == "wave", ref=ref)


# --------------------------------------------------------------------------------------------------------------- e. clips and mask
CLIP_EDGE_DB = 1e-3


def clip_basis(family):
    b = _slaney_lds(80)
    return np.ascontiguousarray(np.tile(b, (13, 1))[:1025]) if family == "banded" else b         # 1025 Slaney rows: the banded kernel's shape


@functools.lru_cache(maxsize=None)
def clip_waveform(kind):
    w = make_waveform(1, 16384, tag="routes.clip")
    if kind == "floor":
        w[:, 4000:9000] = 0.0
    else:
        w = (np.float32(40.0) * w).astype(np.float32)
    w.setflags(write=False)
    return w


def clip_launch(kind, family, mask=None):
    wav = clip_waveform(kind)
    fam_args = dict(misalign=family == "wave")             # an even length one float off alignment: the wave kernel
    return launch(wav, window32(1024, 256, False), clip_basis(family), 256, -100.0, 20.0, family, mask=mask, **fam_args)


@pytest.mark.parametrize("family", ["r512", "wave", "banded", "dense"])
@pytest.mark.parametrize("kind", ["floor", "ceiling"])
def test_both_clips_are_exact(kind, family):
    """elements the fp64 reference puts more than 1e-3 dB beyond a clip point are exactly 0.0 / 1.0; those within 1e-3 dB of one (at most 1 %) are
    left out; the rest is compared on the normalised scale as in test_real_basis"""
    wav, win, basis = clip_waveform(kind), window32(1024, 256, False), clip_basis(family)
    ref_nrm, mag, raw = ref64(wav, win, basis, 1024, 256, -100.0, 20.0)
    lo_pt, hi_pt = -100.0, 0.0
    below, above = raw < lo_pt - CLIP_EDGE_DB, raw > hi_pt + CLIP_EDGE_DB
    edge = (np.abs(raw - lo_pt) <= CLIP_EDGE_DB) | (np.abs(raw - hi_pt) <= CLIP_EDGE_DB)
    assert edge.mean() <= 0.01, edge.mean()
    assert np.all(ref_nrm[below] == 0.0) and np.all(ref_nrm[above] == 1.0)
    if kind == "floor":
        assert below.mean() > 0.2 and int((mag.max(2) == 0).sum()) >= 16, (below.mean(), int((mag.max(2) == 0).sum()))     # the silenced span: whole frames of zeros
    else:
        assert above.mean() > 0.05, above.mean()
    got = clip_launch(kind, family)
    print("clip %-8s family %-6s reference: %.1f %% on the floor, %.1f %% on the ceiling, %.3f %% within %.0e dB of a clip point (left out)" % (
        kind, family, 100 * below.mean(), 100 * above.mean(), 100 * edge.mean(), CLIP_EDGE_DB))
    assert np.all(zero_bits(got[below])), "%d elements below the floor are not bitwise 0.0" % int((~zero_bits(got[below])).sum())
    assert np.all(got[above] == 1.0), "%d elements above the ceiling are not 1.0" % int((got[above] != 1.0).sum())
    mid = ~(below | above | edge)
    cal = float(np.abs(pipe32(wav, win, basis, 1024, 256, -100.0, 20.0).astype(np.float64) - ref_nrm)[mid].max())
    bound = min(2e-4, max(MARGIN * cal, 2.0 * EPS32))
    worst = float(np.abs(got.astype(np.float64) - ref_nrm)[mid].max())
    print("clip %-8s family %-6s unclipped elements: fp32 restatement %.3e  bound %.3e  kernel worst %.3e  ratio %.2f" % (kind, family, cal, bound, worst, worst / bound))
    assert worst <= bound, (worst, bound)
    assert not np.isnan(got).any() and got.min() >= 0.0 and got.max() <= 1.0


@pytest.mark.parametrize("family", ["r512", "wave", "banded", "dense"])
def test_mask_is_a_bitwise_product(family):
    """a non-binary mask: out = unmasked * mask in fp32, bit for bit, over 67 frames = two full 32-frame tiles and one of 3 (8-frame blocks: 8 and 3)"""
    frames = A.lws_num_frames(16384, 1024, 256)
    assert frames == 67
    mask = np.array([0.0, 0.5, 1.0, 0.3], np.float32)[(np.arange(frames) * 7 + np.arange(frames) // 5) % 4][None, :]
    assert len(np.unique(mask)) == 4 and np.all(mask[0, 64:] != 1.0) and np.any(mask[0, 64:] != 0.0)      # the last tile is scaled, not copied
    plain = clip_launch("floor", family)
    masked = clip_launch("floor", family, mask=mask)
    want = plain * mask[:, None, :]
    assert not np.isnan(plain).any()
    assert np.array_equal(masked.view(np.int32), want.astype(np.float32).view(np.int32)), int((masked.view(np.int32) != want.view(np.int32)).sum())
