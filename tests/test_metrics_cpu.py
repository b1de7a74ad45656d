"""Inpainting quality metrics (`viai_amd.metrics`, csrc/metrics.hip), the parts that need no GPU: the C symbols and their refusals, the argument
checks in front of the device, the loud failure on CPU tensors, and the derived figures -- plain torch on the rows of sums -- against their closed
forms."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import metrics_common as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"viai_metrics_ws_doubles": (C.c_long, 5), "viai_wave_gap_stats": (C.c_int, 9), "viai_mel_frame_stats": (C.c_int, 11),
       "viai_mel_ssim": (C.c_int, 14)}
WAVE, FRAMES, SSIM = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    from viai_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_new_symbols_are_declared_typed_and_exported(lib):
    from viai_amd import _lib
    with open(os.path.join(ROOT, "include", "viai_hip.h")) as f:
        header = f.read()
    for name, (res, nargs) in NEW.items():
        got_res, args = _lib.SIGNATURES[name]
        assert got_res is res and len(args) == nargs, name
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args)
        assert ("%s %s(" % ("long" if res is C.c_long else "int", name)) in header
    assert lib.viai_abi_version() == 20 == _lib.ABI_VERSION
    assert "metrics.hip" in open(os.path.join(ROOT, "vision-infused-audio-inpainter-viai_amd", "csrc", "Makefile")).read()
    for k, v in (("VIAI_METRIC_WAVE", WAVE), ("VIAI_METRIC_MEL_FRAMES", FRAMES), ("VIAI_METRIC_MEL_SSIM", SSIM)):
        assert ("#define %s %d" % (k, v)) in header


def test_workspace_query_is_host_arithmetic(lib):
    ws = lib.viai_metrics_ws_doubles
    assert ws(WAVE, 1, 1, 0, 0) == 4 and ws(WAVE, 1, 2048, 0, 0) == 4 and ws(WAVE, 1, 2049, 0, 0) == 8
    assert ws(WAVE, 8, 65536, 0, 0) == 8 * 32 * 4
    assert ws(FRAMES, 3, 80, 37, 0) == 3 * 4 and ws(FRAMES, 8, 80, 259, 0) == 8 * 5 * 4 and ws(FRAMES, 1, 5, 64, 0) == 4
    # SSIM: 16 x 32 tiles over the (F - taps + 1) x (T - taps + 1) valid positions
    assert ws(SSIM, 1, 11, 11, 11) == 2 and ws(SSIM, 1, 12, 300, 11) == 2 * 10 and ws(SSIM, 3, 80, 37, 11) == 3 * 2 * 5
    assert ws(SSIM, 8, 80, 259, 11) == 8 * 2 * 5 * 8 and ws(SSIM, 1, 80, 37, 7) == 2 * 5
    for bad in ((WAVE, 0, 8, 0, 0), (WAVE, 1, 0, 0, 0), (FRAMES, 1, 80, 0, 0), (SSIM, 1, 10, 37, 11), (SSIM, 1, 80, 10, 11), (SSIM, 1, 80, 37, 10),
                (SSIM, 1, 80, 37, 33), (3, 1, 8, 8, 3)):
        assert ws(*bad) == 0, bad


def test_refused_shapes_return_invalid_value_before_any_launch(lib):
    inval, one = 1, 16                                    # hipErrorInvalidValue; a stand-in for a device pointer that is never followed
    wave, frames, ssim = lib.viai_wave_gap_stats, lib.viai_mel_frame_stats, lib.viai_mel_ssim
    assert wave(one, one, one, one, one, one, 1, 0, None) == inval                              # n < 1
    assert wave(one, one, one, one, one, one, 0, 8, None) == inval                              # B < 1
    for k in range(6):                                                                          # every pointer is required
        p = [one] * 6
        p[k] = None
        assert wave(*p, 1, 8, None) == inval, k
    assert wave(one, one, one, one, 20, one, 1, 8, None) == inval                               # out is no double pointer
    assert frames(one, one, one, one, one, 1, 0, 8, 1, 100.0, None) == inval                    # F < 1
    assert frames(one, one, one, one, one, 1, 8, 0, 1, 100.0, None) == inval                    # T < 1
    assert frames(one, one, one, one, one, 0, 8, 8, 1, 100.0, None) == inval
    assert frames(one, one, None, one, one, 1, 8, 8, 1, 100.0, None) == inval                   # where != 0 needs the mask
    assert frames(one, one, None, one, one, 1, 8, 8, 2, 100.0, None) == inval
    assert frames(one, one, one, one, one, 1, 8, 8, 3, 100.0, None) == inval                    # where outside 0 .. 2
    assert frames(one, None, one, one, one, 1, 8, 8, 0, 100.0, None) == inval
    assert frames(one, one, one, one, None, 1, 8, 8, 0, 100.0, None) == inval                   # the workspace is required
    c1, c2 = 1e-4, 9e-4
    assert ssim(one, one, one, one, one, one, 1, 10, 37, 11, 0, c1, c2, None) == inval          # F < taps
    assert ssim(one, one, one, one, one, one, 1, 80, 10, 11, 0, c1, c2, None) == inval          # T < taps
    assert ssim(one, one, one, one, one, one, 1, 80, 37, 10, 0, c1, c2, None) == inval          # even taps
    assert ssim(one, one, one, one, one, one, 1, 80, 80, 33, 0, c1, c2, None) == inval          # taps > 31
    assert ssim(one, one, None, one, one, one, 1, 80, 37, 11, 1, c1, c2, None) == inval         # where != 0 needs the mask
    assert ssim(one, one, one, None, one, one, 1, 80, 37, 11, 0, c1, c2, None) == inval         # the window is required
    assert ssim(one, one, one, one, None, one, 1, 80, 37, 11, 0, c1, c2, None) == inval
    assert ssim(one, one, one, one, one, one, 0, 80, 37, 11, 0, c1, c2, None) == inval


def test_argument_errors_are_raised_before_the_device():
    from viai_amd import metrics as M
    x = torch.zeros(2, 100)
    with pytest.raises(ValueError, match="differ in shape"):
        M.wave_gap_stats(x, torch.zeros(2, 101), 3, 4)
    with pytest.raises(ValueError, match=r"\(B, n\)"):
        M.wave_gap_stats(torch.zeros(100), torch.zeros(100), 3, 4)
    for start, length in ((-1, 10), (10, -1), (95, 6), ([0, 100], [1, 1])):
        with pytest.raises(ValueError, match="inside the clip's 100 samples"):
            M.wave_gap_stats(x, x, start, length)
    with pytest.raises(ValueError, match="per stream"):
        M.wave_gap_stats(x, x, [1, 2, 3], 4)
    mel = torch.zeros(2, 1, 12, 20)
    mask = torch.ones(2, 1, 1, 20)
    for fn in (M.mel_frame_stats, M.mel_ssim):
        with pytest.raises(ValueError, match="differ in shape"):
            fn(mel, torch.zeros(2, 1, 12, 21), mask)
        with pytest.raises(ValueError, match="needs the"):
            fn(mel, mel)                                                  # the default is "damaged"
        with pytest.raises(ValueError, match="needs the"):
            fn(mel, mel, None, "clean")
        with pytest.raises(ValueError, match="where is"):
            fn(mel, mel, mask, "gap")
        with pytest.raises(ValueError, match=r"mask is \(B, 1, 1, T\)"):
            fn(mel, mel, torch.ones(2, 1, 1, 19))
        with pytest.raises(ValueError, match=r"\(B, 1, F, T\)"):
            fn(mel[:, 0], mel[:, 0], mask)
    for win in (10, 0, 33):
        with pytest.raises(ValueError, match="win is odd"):
            M.mel_ssim(mel, mel, mask, win=win)
    with pytest.raises(ValueError, match="holds no 13 x 13 window"):
        M.mel_ssim(mel, mel, mask, win=13)                               # F < win
    with pytest.raises(ValueError, match="holds no 11 x 11 window"):
        M.mel_ssim(torch.zeros(1, 1, 12, 10), torch.zeros(1, 1, 12, 10), None, "all")          # T < win


def test_cpu_tensors_fail_loudly():
    from viai_amd import metrics as M
    from viai_amd._lib import ViaiLibraryError
    x = torch.zeros(2, 100)
    mel = torch.zeros(2, 1, 12, 20)
    mask = torch.ones(2, 1, 1, 20)
    with pytest.raises(ViaiLibraryError, match="GPU only; no CPU fallback"):
        M.wave_gap_stats(x, x, [0, 99], [100, 1])
    with pytest.raises(ViaiLibraryError, match="GPU only; no CPU fallback"):
        M.mel_frame_stats(mel, mel, mask)
    with pytest.raises(ViaiLibraryError, match="GPU only; no CPU fallback"):
        M.mel_frame_stats(mel, mel, None, "all")
    with pytest.raises(ViaiLibraryError, match="GPU only; no CPU fallback"):
        M.mel_ssim(mel, mel, mask)


def test_the_module_is_reached_by_its_own_name_only():
    import viai_amd
    from viai_amd import metrics as M
    for name in ("wave_gap_stats", "snr_db", "si_sdr_db", "mel_frame_stats", "mel_l1", "mel_psnr_db", "mel_lsd_db", "mel_ssim", "inpainting_report"):
        assert callable(getattr(M, name))
        with pytest.raises(AttributeError):
            getattr(viai_amd, name)


def test_snr_and_si_sdr_are_the_closed_forms():
    from viai_amd import metrics as M
    rng = np.random.default_rng(7)
    ref = rng.standard_normal(500)
    rows, want_snr, want_sdr = [], [], []
    for scale, noise in ((1.0, 0.1), (0.5, 0.0), (2.0, 1.0), (-1.0, 0.01)):
        est = scale * ref + noise * rng.standard_normal(500)
        s, _ = R.wave_gap_stats(ref, est, 17, 301)
        rows.append(s)
        x, y = ref[17:318], est[17:318]
        want_snr.append(10 * math.log10((x ** 2).sum() / ((x - y) ** 2).sum()))
        alpha = (x * y).sum() / (x * x).sum()                             # the definition, from the signals
        want_sdr.append(10 * math.log10(((alpha * x) ** 2).sum() / ((y - alpha * x) ** 2).sum()) if noise else None)
    rows.append(np.zeros(5))                                             # an empty gap
    stats = torch.tensor(np.stack(rows))
    snr, sdr = M.snr_db(stats), M.si_sdr_db(stats)
    assert snr.dtype == torch.float64 and tuple(snr.shape) == (5,) and tuple(sdr.shape) == (5,)
    for k in range(4):
        assert abs(float(snr[k]) - want_snr[k]) < 1e-9 and abs(float(snr[k]) - R.snr_db(rows[k])) < 1e-9
        if want_sdr[k] is not None:
            assert abs(float(sdr[k]) - want_sdr[k]) < 1e-6 and abs(float(sdr[k]) - R.si_sdr_db(rows[k])) < 1e-9
    assert math.isnan(float(snr[4])) and math.isnan(float(sdr[4]))
    assert abs(float(snr[1]) - 10 * math.log10(4.0)) < 1e-9              # est = ref / 2: the error is ref / 2
    assert float(sdr[3]) > 35 and float(snr[3]) < -5.9                   # est = -ref: the scale, sign included, is forgiven by SI-SDR only
    # hand-made rows: ref = (3, 4), est = (3, 0)  ->  25, 9, 16, 9
    hand = torch.tensor([[2.0, 25.0, 9.0, 16.0, 9.0]])
    assert abs(float(M.snr_db(hand)[0]) - 10 * math.log10(25 / 16)) < 1e-12
    a = 9 / 25
    assert abs(float(M.si_sdr_db(hand)[0]) - 10 * math.log10(a * a * 25 / (9 - 2 * a * 9 + a * a * 25))) < 1e-12


def test_mel_figures_from_rows_are_the_closed_forms():
    from viai_amd import metrics as M
    rng = np.random.default_rng(11)
    F, T = 6, 9
    ref, est = rng.random((F, T)), rng.random((F, T))
    mask = np.ones(T)
    mask[[2, 5, 6]] = 0
    rows = [R.mel_frame_stats(ref, est, mask, w)[0] for w in R.WHERE] + [R.mel_frame_stats(ref, est, np.ones(T), "damaged")[0]]
    assert [int(r[0]) for r in rows] == [9, 3, 6, 0]
    stats = torch.tensor(np.stack(rows))
    l1, psnr, lsd = M.mel_l1(stats, F), M.mel_psnr_db(stats, F), M.mel_lsd_db(stats)
    d = est - ref
    sel = mask == 0
    assert abs(float(l1[1]) - np.abs(d[:, sel]).mean()) < 1e-12
    assert abs(float(psnr[1]) - 10 * math.log10(1 / (d[:, sel] ** 2).mean())) < 1e-9
    assert abs(float(lsd[1]) - np.sqrt(((100 * d[:, sel]) ** 2).mean(0)).mean()) < 1e-9
    for k in range(3):
        assert abs(float(l1[k]) - R.mel_l1(rows[k], F)) < 1e-12 and abs(float(psnr[k]) - R.mel_psnr_db(rows[k], F)) < 1e-9
        assert abs(float(lsd[k]) - R.mel_lsd_db(rows[k])) < 1e-9
    assert all(math.isnan(float(v[3])) for v in (l1, psnr, lsd))


def test_the_window_is_the_normalised_gaussian():
    from viai_amd import metrics as M
    for win, sigma in ((11, 1.5), (7, 1.0), (31, 4.0), (1, 1.5)):
        g = M.gaussian_window(win, sigma)
        assert len(g) == win and abs(math.fsum(g) - 1) < 1e-15 and g == g[::-1]
        assert np.abs(np.array(g) - R.gaussian(win, sigma)).max() < 2e-16


def test_reference_ssim_of_an_image_with_itself_is_one():
    rng = np.random.default_rng(3)
    x = rng.random((14, 15)).astype(np.float32)
    g = R.gaussian()
    m = R.ssim_map(x, x, g, 1e-4, 9e-4)
    assert m.shape == (4, 5) and np.abs(m - 1).max() < 1e-12
    mask = np.ones(15)
    mask[[0, 5, 9, 14]] = 0                                               # 0 and 14 are no centre; 5 and 9 are the first and the last
    assert R.mel_ssim(x, x, mask, "damaged", g)[0] == 2 * 4 and R.mel_ssim(x, x, mask, "clean", g)[0] == 3 * 4
    assert R.mel_ssim(x, x, None, "all", g)[0] == 20
