"""The inpainting metrics restated in fp64 numpy, one formula per function, for tests/test_metrics_*.py.  Every function takes one stream (the
batch is a Python loop in the caller) and returns the SUMS the kernels return, plus `abs_terms`, the sum of the terms' magnitudes that the
tolerance of a reordered fp64 sum is stated against."""
import numpy as np

WHERE = ("all", "damaged", "clean")


def selected(mask_row, where, T):
    """bool (T,): the frames `where` selects against a (T,) time mask (1 = known, 0 = damaged); mask_row None: every frame"""
    if where == "all" or mask_row is None:
        assert where == "all"
        return np.ones(T, dtype=bool)
    m = np.asarray(mask_row, dtype=np.float64).reshape(T)
    return m == 0 if where == "damaged" else m != 0


def wave_gap_stats(ref, est, g0, glen):
    """ref, est (n,) -> ({count, sum ref^2, sum est^2, sum (ref - est)^2, sum ref est}, abs_terms) over [g0, g0 + glen)"""
    x = np.asarray(ref, dtype=np.float64)[g0:g0 + glen]
    y = np.asarray(est, dtype=np.float64)[g0:g0 + glen]
    d = x - y
    sums = np.array([float(len(x)), (x * x).sum(), (y * y).sum(), (d * d).sum(), (x * y).sum()])
    mags = np.array([0.0, (x * x).sum(), (y * y).sum(), (d * d).sum(), np.abs(x * y).sum()])
    return sums, mags


def snr_db(s):
    return 10.0 * np.log10(s[1] / s[3]) if s[0] > 0 else float("nan")


def si_sdr_db(s):
    """target alpha ref, distortion est - alpha ref, alpha = <ref, est> / <ref, ref>"""
    if not s[0] > 0:
        return float("nan")
    alpha = s[4] / s[1]
    return 10.0 * np.log10(alpha * alpha * s[1] / (s[2] - 2.0 * alpha * s[4] + alpha * alpha * s[1]))


def mel_frame_stats(ref, est, mask_row, where, db_range=100.0):
    """ref, est (F, T) -> ({frames, sum |d|, sum d^2, sum_t sqrt(mean_f (db_range d)^2)}, abs_terms) over the selected frames, d = est - ref"""
    x, y = np.asarray(ref, dtype=np.float64), np.asarray(est, dtype=np.float64)
    F, T = x.shape
    sel = selected(mask_row, where, T)
    d = (y - x)[:, sel]
    lsd = np.sqrt(((db_range * d) ** 2).mean(axis=0)) if d.shape[1] else np.zeros(0)
    sums = np.array([float(sel.sum()), np.abs(d).sum(), (d * d).sum(), lsd.sum()])
    return sums, np.array([0.0, sums[1], sums[2], sums[3]])


def mel_l1(s, F):
    return s[1] / (s[0] * F) if s[0] > 0 else float("nan")


def mel_psnr_db(s, F):
    return 10.0 * np.log10(1.0 / (s[2] / (s[0] * F))) if s[0] > 0 else float("nan")


def mel_lsd_db(s):
    return s[3] / s[0] if s[0] > 0 else float("nan")


def gaussian(win=11, sigma=1.5):
    g = np.exp(-((np.arange(win) - win // 2) ** 2) / (2.0 * sigma ** 2))
    return g / g.sum()


def ssim_map(ref, est, g, c1, c2):
    """Wang et al.'s SSIM of two (F, T) images in "valid" mode: a direct 2-D correlation with outer(g, g), population moments.
    Entry (f, t) is the window whose corner is (f, t) and whose centre is (f + win // 2, t + win // 2)."""
    x, y = np.asarray(ref, dtype=np.float64), np.asarray(est, dtype=np.float64)
    g = np.asarray(g, dtype=np.float64)
    k = len(g)
    w2 = np.outer(g, g)
    F, T = x.shape
    PF, PT = F - k + 1, T - k + 1

    def corr(a):
        out = np.zeros((PF, PT))
        for i in range(k):
            for j in range(k):
                out += w2[i, j] * a[i:i + PF, j:j + PT]
        return out
    mx, my = corr(x), corr(y)
    vx, vy, cxy = corr(x * x) - mx * mx, corr(y * y) - my * my, corr(x * y) - mx * my
    return ((2.0 * mx * my + c1) * (2.0 * cxy + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2))


def mel_ssim(ref, est, mask_row, where, g, data_range=1.0):
    """(positions counted, mean ssim or nan) over the positions whose CENTRE frame is selected"""
    k = len(g)
    T = np.asarray(ref).shape[1]
    m = ssim_map(ref, est, g, (0.01 * data_range) ** 2, (0.03 * data_range) ** 2)
    sel = selected(mask_row, where, T)[k // 2:T - k // 2]
    count = int(sel.sum()) * m.shape[0]
    return count, (m[:, sel].sum() / count if count else float("nan"))
