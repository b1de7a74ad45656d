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

# The launch forms RATIOS does not reach (all six are the period form, pp = 4, with spans of at most 5426 words): rates -> ((L, M, H, T),
# (pp, lt, g, span)) as `pick` below states the rule.  Kept apart from RATIOS: the tests that iterate over RATIOS use sizes that would be slow here.
FORMS = {
    (11025, 16000): ((640, 441, 24, 49), (1, 1024, 1, 755)),             # L > 512: the consecutive form, up
    (11025, 48000): ((640, 147, 24, 49), (1, 1024, 1, 285)),
    (16001, 16000): ((16000, 16001, 25, 51), (1, 1024, 1, 1076)),        # a period far longer than a tile
    (4001, 400): ((400, 4001, 241, 483), (1, 1024, 1, 10717)),           # L <= 512, but one period of four outputs per item does not fit
    (8337, 521): ((521, 8337, 385, 771), (1, 512, 1, 8949)),             # shorter consecutive tiles as M / L grows
    (28135, 521): ((521, 28135, 1297, 2595), (1, 256, 1, 16367)),        # 17 words under the budget: 65 468 bytes of LDS
    (36471, 521): ((521, 36471, 1681, 3363), (1, 128, 1, 12255)),
    (62521, 521): ((521, 62521, 2881, 5763), (1, 64, 1, 13325)),
    (300, 1): ((1, 300, 7200, 14401), (4, 1, 1, 15303)),                 # the period form with one work item per block, 61 KB of LDS
}
REFUSED = {(330, 1): (1, 330, 7920, 15841), (44100, 100): (1, 441, 10584, 21169),      # a valid table and no tile that fits: L <= 512 ...
           (77109, 521): (521, 77109, 3553, 7107)}                                     # ... and L > 512
PERIOD_FORMS = {(44100, 16000): (4, 160, 3, 5426), (16000, 44100): (4, 441, 1, 690), (48000, 16000): (4, 1, 254, 3192),
                (16000, 48000): (4, 3, 85, 390), (22050, 16000): (4, 320, 3, 5361), (16000, 22050): (4, 441, 1, 1330)}


def plan(sr_in, sr_out, zeros=ZEROS):
    g = math.gcd(sr_in, sr_out)
    L, M = sr_out // g, sr_in // g
    H = -(-zeros * M // L) if M > L else zeros                           # ceil(zeros / min(1, L / M)), in integers
    return L, M, H, 2 * H + 1


THREADS, PP, MAX_SPAN, PERIOD_MAX_L, MAX_TABLE = 256, 4, 16384, 512, 1 << 22


def span(tile_len, L, M, H):
    """the input samples a tile of tile_len consecutive outputs stages: i0 moves by at most floor((tile_len - 1) M / L) + 1 inside it"""
    return (tile_len - 1) * M // L + 2 * H + 3


def pick(L, M, H):
    """(pp, lt, g, span): the launch form of a plan, the rule of csrc/wav_resample.hip restated.  A tile is lt g pp consecutive outputs.
    pp = 4, lt = L: the period form for L <= 512, g = 1 when its span fits and a larger g <= max(1, 1024 // L) only where L g fills passes of
    256 lanes better by more than a hundredth; pp = 1, g = 1: the consecutive form, the largest lt of 1024 .. 64 whose span fits; (0, 0, 0, 0):
    no tile fits the 16 384 words."""
    if L <= PERIOD_MAX_L:
        best, full = None, None
        for g in range(1, max(1, 1024 // L) + 1):
            items = L * g
            words = span(items * PP, L, M, H)
            if words > MAX_SPAN:
                break
            slots = -(-items // THREADS) * THREADS
            if g == 1 or items * full[1] * 100 > full[0] * slots * 101:
                best, full = (PP, L, g, words), (items, slots)
        if best is not None:
            return best
    for lt in (1024, 512, 256, 128, 64):
        if span(lt, L, M, H) <= MAX_SPAN:
            return 1, lt, 1, span(lt, L, M, H)
    return 0, 0, 0, 0


def value_size(rates):
    """(n, m) for a value test of a plan of FORMS: a little over two tiles of the plan's own tile and a ragged tail, at most a few thousand
    outputs, and a clip long enough to hold whole filters (2 T + 5 samples)"""
    (L, M, H, T), (pp, lt, g, _) = FORMS[rates]
    tile = pp * lt * g
    n = max((2 * tile + tile // 3 + 2) * M // L, 2 * T + 5)
    return n, out_len(n, L, M)


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
