"""The autoregressive gap fill of include/viai_hip.h ("short gaps") restated in numpy fp64 with ordinary np.dot sums, and the cases
tests/test_ar_fill_cpu.py and tests/test_ar_fill_gpu.py share.

The restatement does NOT reproduce the rule's summation order (256 strided partials and a pairwise tree): it is a second opinion on the method,
not a copy of the kernel.  The host mirror `ar_fill_host` is compared with it under a tolerance; the device is compared with the host mirror
bit for bit.

    skipped     L < 1, L > max_len, s < 0, e > len                                    -> filled 0, nothing written
    contexts    [max(s - context, end of gap k-1, 0), s) and [e, min(e + context, start of gap k+1, len)); non-finite samples read as 0
    order       p = min(order, C // 2) per side, usable iff p >= 1
    fit         Burg: f = x[1:], b = x[:-1]; k = -2 f.b / (f.f + b.b) (0 when the denominator is 0); a <- [a, 0] + k reverse([a, 0])
    extrapolate x^[i] = -sum_j a_j x^[i-j], forward from the left, backward from the right (the right context time-reversed)
    blend       u = (i + 0.5) / L, w = 1 - u u (3 - 2 u), out = w fwd + (1 - w) bwd, one rounding to fp32

A case is a dict: name, wav (B, stride) float32 with the clip in its first n columns, n, lengths (or None), gaps (count, start, length) and the
keyword arguments order / context / max_len.  Signals come from `viai_amd.synth.uniform` (integer-hash draws): no RNG state anywhere."""
import math

import numpy as np

RATE = 16000


# ------------------------------------------------------------------------------------------------------------------------------ the rule
def burg(x, p):
    """coefficients a[0 .. p] of Burg's method on x"""
    x = np.asarray(x, dtype=np.float64)
    f, b = x[1:].copy(), x[:-1].copy()
    a = np.array([1.0])
    for _ in range(p):
        den = np.dot(f, f) + np.dot(b, b)
        k = 0.0 if den == 0.0 else -2.0 * np.dot(f, b) / den
        a0 = np.concatenate((a, [0.0]))
        a = a0 + k * a0[::-1]
        f, b = (f + k * b)[1:], (b + k * f)[:-1]
    return a


def extrapolate(a, ctx, L):
    p = len(a) - 1
    buf = np.concatenate((np.asarray(ctx, dtype=np.float64)[len(ctx) - p:], np.zeros(L)))
    for i in range(L):
        buf[p + i] = -np.dot(a[1:], buf[i:p + i][::-1])
    return buf[p:]


def finite64(x):
    x = np.asarray(x, dtype=np.float64).copy()
    x[~np.isfinite(x)] = 0.0
    return x


def fill_rule(wav, n, gaps, lengths=None, order=32, context=1024, max_len=4096):
    """-> (out (B, n) float32, filled (B, K) int32)"""
    count, start, length = (np.asarray(g) for g in gaps)
    B, K = start.shape
    out = np.array(wav[:, :n], dtype=np.float32, copy=True)
    filled = np.zeros((B, K), dtype=np.int32)
    for b in range(B):
        ln = n if lengths is None else min(max(int(lengths[b]), 0), n)
        listed = min(max(int(count[b]), 0), K)
        row = wav[b]
        for k in range(listed):
            s, L = int(start[b, k]), int(length[b, k])
            e = s + L
            if L < 1 or L > max_len or s < 0 or e > ln:
                continue
            lo = max(s - context, 0)
            if k > 0:
                lo = max(lo, int(start[b, k - 1]) + int(length[b, k - 1]))
            hi = min(e + context, ln)
            if k + 1 < listed:
                hi = min(hi, int(start[b, k + 1]))
            left, right = finite64(row[lo:s]) if lo < s else np.zeros(0), finite64(row[e:hi])[::-1] if hi > e else np.zeros(0)
            pl, pr = min(order, len(left) // 2), min(order, len(right) // 2)
            fwd = extrapolate(burg(left, pl), left, L) if pl >= 1 else None
            bwd = extrapolate(burg(right, pr), right, L)[::-1] if pr >= 1 else None
            if fwd is not None and bwd is not None:
                u = (np.arange(L) + 0.5) / L
                w = 1.0 - u * u * (3.0 - 2.0 * u)
                val, code = w * fwd + (1.0 - w) * bwd, 1
            elif fwd is not None:
                val, code = fwd, 2
            elif bwd is not None:
                val, code = bwd, 3
            else:
                val, code = np.zeros(L), 4
            with np.errstate(over="ignore"):
                out[b, s:e] = val.astype(np.float32)
            filled[b, k] = code
    return out, filled


_EXPECTED = {}


def expected(case):
    if case["name"] not in _EXPECTED:
        got = fill_rule(case["wav"], case["n"], case["gaps"], case["lengths"], **case["kw"])
        for a in got:
            a.setflags(write=False)
        _EXPECTED[case["name"]] = got
    return _EXPECTED[case["name"]]


def gap_snr_db(ref, est, spans):
    """10 log10(sum ref^2 / sum (ref - est)^2) over the samples of `spans` [(s, e)] of one row, fp64"""
    idx = np.concatenate([np.arange(s, e) for s, e in spans])
    r, d = ref[idx].astype(np.float64), ref[idx].astype(np.float64) - est[idx].astype(np.float64)
    return 10.0 * math.log10(np.dot(r, r) / np.dot(d, d))


# ------------------------------------------------------------------------------------------------------------------------------ the signals
def draws(tag, shape, lo, hi):
    from viai_amd import synth
    return synth.uniform(tag, shape, lo, hi).numpy().astype(np.float64)


def tones(tag, B, n, sigma=0.0, freqs=None):
    """(B, n) float32: three sinusoids of amplitude 0.2 per row, 100 - 4000 Hz at 16 kHz (drawn per row unless `freqs` (B, 3) is given), random
    phases, plus uniform noise of standard deviation sigma"""
    f = draws(tag + ".f", (B, 3), 100.0, 4000.0) if freqs is None else np.asarray(freqs, dtype=np.float64).reshape(B, 3)
    ph = draws(tag + ".p", (B, 3), 0.0, 2.0 * math.pi)
    t = np.arange(n, dtype=np.float64)[None, :] / RATE
    y = np.zeros((B, n))
    for j in range(3):
        y += 0.2 * np.sin(2.0 * math.pi * f[:, j:j + 1] * t + ph[:, j:j + 1])
    if sigma > 0:
        y += sigma * math.sqrt(3.0) * draws(tag + ".n", (B, n), -1.0, 1.0)
    return y.astype(np.float32)


def lists(rows, K):
    """[(s, L), ...] per row -> (count, start, length) int32 with K columns; a row may hold more than K entries (count says so)"""
    B = len(rows)
    count = np.array([len(r) for r in rows], dtype=np.int32)
    start = np.zeros((B, K), dtype=np.int32)
    length = np.zeros((B, K), dtype=np.int32)
    for b, r in enumerate(rows):
        for k, (s, L) in enumerate(r[:K]):
            start[b, k], length[b, k] = s, L
    return count, start, length


def damage(wav, rows, value=0.0):
    """a copy of wav with `value` written into every listed [s, s + L) that lies inside the row"""
    hurt = wav.copy()
    for b, r in enumerate(rows):
        for s, L in r:
            if L > 0 and s >= 0:
                hurt[b, s:s + L] = value
    return hurt


def case(name, wav, gaps, n=None, lengths=None, **kw):
    kw.setdefault("order", 32)
    kw.setdefault("context", 1024)
    kw.setdefault("max_len", 4096)
    return {"name": name, "wav": wav, "n": wav.shape[1] if n is None else n, "lengths": lengths, "gaps": gaps, "kw": kw}


# ------------------------------------------------------------------------------------------------------------------------------ the cases
def _build():
    out = []
    # three gaps per row at the issue's lengths, n not a multiple of anything
    rows = [[(700, 64), (2200, 100), (3900, 160)], [(1500, 160), (3000, 64), (4100, 100)], [(1100, 100)]]
    out.append(case("three gaps a row", damage(tones("ar.basic", 3, 5000, 0.01), rows), lists(rows, 4)))
    # the row's ends: code 3, code 2, code 4, and one context sample on a side (unusable: p = 1 // 2 = 0)
    n = 2048
    rows = [[(0, 80)], [(n - 90, 90)], [(0, n)], [(1, 70), (n - 61, 60)]]
    out.append(case("row ends", damage(tones("ar.ends", 4, n, 0.01), rows), lists(rows, 2), max_len=n))
    # two and three context samples: p = 1
    rows = [[(2, 40), (45, 30)], [(300, 50), (352, 20), (374, 10)]]
    out.append(case("tiny contexts", damage(tones("ar.tiny", 2, 600, 0.01), rows), lists(rows, 3), order=8, context=64))
    # lengths shorter than n in wider rows: the right context stops at len, a gap that crosses len or lies behind it is skipped
    n, stride = 3000, 3011
    rows = [[(900, 120), (2500, 100)], [(900, 120), (2500, 100)], [(900, 120), (2500, 100)], [(900, 120)]]
    wav = damage(tones("ar.ragged", 4, stride, 0.01), rows)
    out.append(case("ragged rows", wav, lists(rows, 2), n=n, lengths=np.array([2700, 2550, 2400, -5], dtype=np.int32)))
    out.append(case("ragged rows, no lengths", wav, lists(rows, 2), n=n))
    # neighbours: 10 apart, touching, and a skipped neighbour (longer than max_len) that still bounds the context
    rows = [[(1000, 100), (1110, 90)], [(800, 64), (864, 64), (928, 64)], [(500, 300), (900, 100), (1100, 64)]]
    out.append(case("neighbours", damage(tones("ar.nb", 3, 2500, 0.01), rows), lists(rows, 3), max_len=256))
    # max_len: L = max_len is filled, L = max_len + 1 is not; and entries that are no gap
    rows = [[(600, 128), (1500, 129)], [(400, 0), (700, -3), (-4, 50), (1200, 64)]]
    out.append(case("max_len and no gaps", damage(tones("ar.max", 2, 2500, 0.01), rows), lists(rows, 4), max_len=128))
    # count > K fills the first K; count = 0 and a negative count touch nothing
    rows = [[(300, 64), (700, 64), (1100, 64), (1500, 64), (1900, 64)], [], [(500, 64)]]
    count, start, length = lists(rows, 3)
    count[2] = -2
    out.append(case("overflow and empty", damage(tones("ar.over", 3, 2400, 0.01), rows), (count, start, length)))
    # the orders at both ends, and both terms of a lane in the extrapolation (p > 64)
    rows = [[(4096, 300)], [(3000, 77), (6000, 200)]]
    wav = damage(tones("ar.order", 2, 8192, 0.01), rows)
    for order, context in ((1, 1024), (2, 2), (65, 4096), (128, 4096), (128, 200)):
        out.append(case("order %d context %d" % (order, context), wav, lists(rows, 2), order=order, context=context))
    # a long gap
    rows = [[(2000, 1024)], [(1500, 513)]]
    out.append(case("long gaps", damage(tones("ar.long", 2, 6000, 0.01), rows), lists(rows, 1)))
    # non-finite and extreme context samples
    rows = [[(1500, 100)], [(1500, 100)]]
    wav = damage(tones("ar.nan", 2, 3000, 0.01), rows)
    wav[0, 1400], wav[0, 1450], wav[0, 1700] = np.float32("nan"), np.float32("inf"), np.float32("-inf")
    wav[1, 1499], wav[1, 1600] = np.float32("nan"), np.float32(-0.0)
    out.append(case("non-finite context", wav, lists(rows, 1)))
    # noiseless rows (the badly conditioned end of the method)
    rows = [[(1200, 64), (2600, 160)], [(2000, 160)]]
    out.append(case("noiseless order 16", damage(tones("ar.clean", 2, 4000), rows), lists(rows, 2), order=16, context=512))
    assert len({c["name"] for c in out}) == len(out)
    for c in out:
        assert c["wav"].shape[0] <= 4 and c["n"] <= 8192
    return out


_CASES = []


def all_cases():
    if not _CASES:
        _CASES.extend(_build())
    return _CASES


def case_names():
    return [c["name"] for c in all_cases()]


def case_by_name(name):
    return next(c for c in all_cases() if c["name"] == name)


def filled_mask(case, filled):
    """(B, n) bool: the samples of the gaps whose code is 1 .. 4"""
    count, start, length = case["gaps"]
    m = np.zeros((case["wav"].shape[0], case["n"]), dtype=bool)
    for b in range(m.shape[0]):
        for k in range(start.shape[1]):
            if filled[b, k] > 0:
                m[b, start[b, k]:start[b, k] + length[b, k]] = True
    return m


def worst_relative_difference(fill):
    """max over the case table of max |fill(case) - restatement| / the row's peak over the filled samples (the others are compared bit by
    bit elsewhere); `fill(wav, gaps, lengths=, **kw)` -> (out, filled)"""
    return max(relative_difference(c, fill(c["wav"][:, :c["n"]], c["gaps"], lengths=c["lengths"], **c["kw"])[0]) for c in all_cases())


def relative_difference(c, got):
    want, filled = expected(c)
    peak = np.max(np.abs(finite64(c["wav"][:, :c["n"]])), axis=1, keepdims=True)
    peak[peak == 0.0] = 1.0                                                  # a row that is one gap: zeros are expected, absolutely
    with np.errstate(invalid="ignore"):                                      # NaN and Inf context samples: outside the mask
        diff = np.abs(got.astype(np.float64) - want.astype(np.float64)) / peak
    m = filled_mask(c, filled)
    return float(np.max(diff[m])) if m.any() else 0.0
