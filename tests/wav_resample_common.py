"""The polyphase resampler restated in fp64 numpy, one formula per function, for tests/test_wav_resample_*.py.

    sr_in -> sr_out: g = gcd, L = sr_out / g, M = sr_in / g, s = min(1, L / M), c = rolloff s, W = zeros / s, H = ceil(W), T = 2 H + 1
    y[k] = sum_j x[i0 - H + j] h_r[j],  i0 = floor(k M / L),  r = (k M) mod L,  h_r[j] = c sinc(c t) kaiser(t / W),  t = r / L - (j - H)

The table here is (L, T) in PERIOD order: row q belongs to the outputs k = q (mod L), i.e. to the phase (q M) mod L.  The library's table is the
transpose (tap-major)."""
import math

import numpy as np

RATIOS = {(44100, 16000): (160, 441, 67, 135), (16000, 44100): (441, 160, 24, 49), (48000, 16000): (1, 3, 72, 145),
          (16000, 48000): (3, 1, 24, 49), (22050, 16000): (320, 441, 34, 69), (16000, 22050): (441, 320, 24, 49)}
ZEROS, ROLLOFF, BETA = 24, 0.945, 8.6


def plan(sr_in, sr_out, zeros=ZEROS):
    g = math.gcd(sr_in, sr_out)
    L, M = sr_out // g, sr_in // g
    H = -(-zeros * M // L) if M > L else zeros                           # ceil(zeros / min(1, L / M)), in integers
    return L, M, H, 2 * H + 1


def out_len(n, L, M):
    return -(-n * L // M)


def table(sr_in, sr_out, zeros=ZEROS, rolloff=ROLLOFF, beta=BETA):
    """(h (L, T) float64 in period order, first (L,) int64)"""
    L, M, H, T = plan(sr_in, sr_out, zeros)
    s = min(1.0, L / M)
    c, W = rolloff * s, zeros / s
    q = np.arange(L, dtype=np.int64)
    r = (q * M) % L
    t = (r / L)[:, None] - (np.arange(T) - H)[None, :]
    u = t / W
    inside = np.abs(u) < 1.0
    kaiser = np.where(inside, np.i0(beta * np.sqrt(np.where(inside, 1.0 - u * u, 0.0))) / np.i0(beta), 0.0)
    return c * np.sinc(c * t) * kaiser, (q * M) // L


def resample(x, L, M, H, h, m=None, dtype=np.float64):
    """x (n,) -> (y (m,), mags (m,)): the formula with the (L, T) table h, x zero outside [0, n); mags[k] = sum_j |x_j| |h_j|, what the error bound
    of a T-term dot product is stated against.  dtype float32: the kernel's chain acc = fma(x, h, acc) in tap order -- the product of two floats is
    exact in a double, so each step is the double sum rounded to fp32."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    n, T = x.size, 2 * H + 1
    m = out_len(n, L, M) if m is None else m
    if n == 0:
        return np.zeros(m, dtype=dtype), np.zeros(m)
    k = np.arange(m, dtype=np.int64)
    i0, q = (k * M) // L, k % L
    idx = i0[:, None] - H + np.arange(T)[None, :]
    ok = (idx >= 0) & (idx < n)
    xs = np.where(ok, x[np.clip(idx, 0, n - 1)], 0.0)
    hs = np.asarray(h)[q]
    mags = (np.abs(xs) * np.abs(hs)).sum(1)
    if dtype is np.float64:
        return (xs * hs).sum(1), mags
    xs, hs = xs.astype(np.float32).astype(np.float64), hs.astype(np.float32).astype(np.float64)
    acc = np.zeros(m, dtype=np.float32)
    for j in range(T):
        acc = (acc.astype(np.float64) + xs[:, j] * hs[:, j]).astype(np.float32)
    return acc, mags


def gap_at_rate(g0, g1, L, M, H, m):
    if g1 <= g0:
        return 0, 0
    k0 = max(0, -(-(g0 - H) * L // M))
    k1 = min(m, -(-(g1 + H) * L // M))
    return (k0, k1) if k1 > k0 else (0, 0)


def support(k, L, M, H):
    """[lo, hi]: the inputs output k reads"""
    i0 = k * M // L
    return i0 - H, i0 + H


def db(err, ref):
    return 10.0 * math.log10(float(np.mean(np.square(err))) / float(np.mean(np.square(ref))) + 1e-300)
