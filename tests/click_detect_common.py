"""The click detector of include/viai_hip.h ("clicks") restated in numpy, twice, and the cases tests/test_click_detect_cpu.py and
tests/test_click_detect_gpu.py share.

    rule_exact      steps FIT .. RUNS with the rule's own summation orders, built on `ar_fit_host`'s coefficients: the residual accumulated in
                    ascending j, the variance sums as 256 strided partials and the adjacent pairwise tree, flags, dilation, and the run rule of
                    `find_gaps_host` applied to the mask.  `find_clicks_host` must equal it as exact integers.
    rule_ordinary   the same method with ordinary sums (np.dot in Burg's recursion, np.convolve, np.sum): a second opinion on the method, not a
                    copy of the kernel.  Compared flag by flag outside a measured margin around the threshold.

The base signal is an AR(2) process with poles 0.97 e^{+-0.2i}, unit Gaussian innovation, 200 samples of burn-in dropped, scaled to peak 0.5,
fp32; clicks are +-20 s at 12 positions of the grid 100, 250, 400, ..., s the standard deviation of the order-32 Burg residual of the first
clean tile.  Every draw comes from numpy.random.default_rng(seed).

A case is a dict: name, wav (B, stride) float32 with the clip in its first n columns, n, lengths (or None) and the keyword arguments."""
import numpy as np

TILE = 4096
PARTS = 256
N_BASE = 2 * TILE + 777
DEFAULTS = dict(order=32, k=5.0, passes=2, guard=2, floor=0.0, min_len=1, merge_within=8, max_gaps=64)


# ------------------------------------------------------------------------------------------------------------------------------ the rule
def finite64(x):
    x = np.asarray(x, dtype=np.float64).copy()
    x[~np.isfinite(x)] = 0.0
    return x


def burg(x, p):
    """Burg's coefficients a[0 .. p] with ordinary dot products"""
    f, b = x[1:].copy(), x[:-1].copy()
    a = np.array([1.0])
    for _ in range(p):
        den = np.dot(f, f) + np.dot(b, b)
        k = 0.0 if den == 0.0 else -2.0 * np.dot(f, b) / den
        a0 = np.concatenate((a, [0.0]))
        a = a0 + k * a0[::-1]
        f, b = (f + k * b)[1:], (b + k * f)[:-1]
    return a


def tree_sum(part):
    part = np.asarray(part, dtype=np.float64)
    while part.size > 1:
        part = part[0::2] + part[1::2]
    return float(part[0])


def strided_sum(q, take):
    """256 strided partials in ascending index from +0.0 (a sample left out adds nothing: q >= 0, so adding +0.0 instead is the same bits),
    then the adjacent pairwise tree; and the count"""
    C = q.size
    pad = np.zeros(-(-C // PARTS) * PARTS)
    pad[:C] = np.where(take, q, 0.0)
    acc = np.zeros(PARTS)
    for row in pad.reshape(-1, PARTS):
        acc = acc + row
    return tree_sum(acc), int(np.count_nonzero(take))


def ordinary_sum(q, take):
    return float(np.sum(q[take])), int(np.count_nonzero(take))


def tile_ratio(xs, t0, C, order, kk, ff, passes, exact):
    """-> (judged (C,) bool, ratio (C,) = q / threshold of the tile's samples; a threshold of 0 gives inf for q > 0 and 0 for q = 0, over
    (C,) bool = judged and q > threshold, the rule's own comparison)"""
    p = min(order, C // 2)
    judged = np.zeros(C, dtype=bool)
    ratio = np.zeros(C)
    if p < 1:
        return judged, ratio, judged.copy()
    if exact:
        from viai_amd.ar_fill import ar_fit_host
        a, pp = ar_fit_host(xs[t0:t0 + C].astype(np.float32), order)          # xs holds fp32 values: the cast is exact
        assert pp == p
        a = a[:p + 1]
    else:
        a = burg(xs[t0:t0 + C], p)
    g = np.arange(t0, t0 + C)
    judged = g >= p
    gj = g[judged]
    if exact:
        e = np.zeros(gj.size)
        for j in range(p + 1):
            e = e + a[j] * xs[gj - j]
    else:
        e = np.convolve(xs[:t0 + C], a)[gj]
    q = np.zeros(C)
    q[judged] = e * e
    total = strided_sum if exact else ordinary_sum
    s, c = total(q, judged)
    var = s / float(c) if c > 0 else 0.0
    for _ in range(passes):
        s, c = total(q, judged & (q <= kk * var))
        if c > 0:
            var = s / float(c)
    thr = kk * max(var, ff)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(thr > 0, q / thr, np.where(q > 0, np.inf, 0.0))
    ratio[~judged] = 0.0
    return judged, ratio, judged & (q > thr)


def row_flags(x, ln, order, k, passes, floor, exact):
    """-> (flags (ln,) bool, judged (ln,) bool, ratio (ln,))"""
    xs = finite64(x[:ln])
    kk, ff = float(np.float32(k)) * float(np.float32(k)), float(np.float32(floor)) * float(np.float32(floor))
    flags = ~np.isfinite(np.asarray(x[:ln], dtype=np.float64))
    judged, ratio = np.zeros(ln, dtype=bool), np.zeros(ln)
    for t0 in range(0, ln, TILE):
        C = min(TILE, ln - t0)
        judged[t0:t0 + C], ratio[t0:t0 + C], over = tile_ratio(xs, t0, C, order, kk, ff, passes, exact)
        flags[t0:t0 + C] |= over
    return flags, judged, ratio


def dilate(flags, guard):
    ln = flags.size
    mask = np.zeros(ln, dtype=bool)
    for j in np.flatnonzero(flags):
        mask[max(0, j - guard):min(ln, j + guard + 1)] = True
    return mask


def row_len(lengths, b, n):
    return n if lengths is None else min(max(int(lengths[b]), 0), n)


def masks(case, exact=True):
    """per row: (mask (len,) bool, flags, judged, ratio)"""
    kw = dict(DEFAULTS, **case["kw"])
    out = []
    for b in range(case["wav"].shape[0]):
        ln = row_len(case["lengths"], b, case["n"])
        flags, judged, ratio = row_flags(case["wav"][b], ln, kw["order"], kw["k"], kw["passes"], kw["floor"], exact)
        out.append((dilate(flags, kw["guard"]), flags, judged, ratio))
    return out


def rule_exact(case):
    """-> Gaps of numpy arrays: the restatement's masks through `find_gaps_host`'s run rule (a masked sample is an exact zero, the others 1.0)"""
    from viai_amd.gap_detect import find_gaps_host
    kw = dict(DEFAULTS, **case["kw"])
    B, n = case["wav"].shape[0], case["n"]
    good = np.ones((B, n), dtype=np.float32)
    for b, (mask, _, _, _) in enumerate(masks(case, exact=True)):
        good[b, :mask.size][mask] = 0.0
    return find_gaps_host(good, lengths=case["lengths"], threshold=0.0, clip=0.0, min_len=kw["min_len"], merge_within=kw["merge_within"],
                          max_gaps=kw["max_gaps"])


# ------------------------------------------------------------------------------------------------------------------------------ the signals
_BASE = {}


def base_signal(seed, n=N_BASE):
    """(clean (n,) float32, s): the AR(2) base signal and the standard deviation of the order-32 Burg residual of its first tile"""
    if (seed, n) not in _BASE:
        rng = np.random.default_rng(seed)
        w = rng.standard_normal(n + 200)
        a1, a2 = 2.0 * 0.97 * np.cos(0.2), -0.97 * 0.97
        y = np.zeros(n + 200)
        for t in range(n + 200):
            y[t] = w[t] + (a1 * y[t - 1] if t >= 1 else 0.0) + (a2 * y[t - 2] if t >= 2 else 0.0)
        y = y[200:]
        clean = (y * (0.5 / np.max(np.abs(y)))).astype(np.float32)
        C = min(TILE, n)
        x = clean[:C].astype(np.float64)
        e = np.convolve(x, burg(x, min(32, C // 2)))[32:C]
        clean.setflags(write=False)
        _BASE[(seed, n)] = (clean, float(np.sqrt(np.mean(e * e))))
    return _BASE[(seed, n)]


def clicked(seed, n=N_BASE, count=12, scale=20.0, at=None):
    """(clean, hurt, positions, s): +-scale s added at `count` positions of the grid 100, 250, 400, ... (or at the positions `at`)"""
    clean, s = base_signal(seed, n)
    rng = np.random.default_rng(1000 + seed)
    grid = np.arange(100, n - 50, 150)
    pos = np.sort(rng.choice(grid, size=count, replace=False)) if at is None else np.asarray(at)
    sign = rng.choice(np.array([-1.0, 1.0]), size=pos.size)
    hurt = clean.copy()
    hurt[pos] = (hurt[pos].astype(np.float64) + sign * scale * s).astype(np.float32)
    return clean, hurt, pos, s


def case(name, wav, n=None, lengths=None, **kw):
    wav = np.ascontiguousarray(wav, dtype=np.float32)
    return {"name": name, "wav": wav, "n": wav.shape[1] if n is None else n, "lengths": None if lengths is None else np.asarray(lengths, np.int32),
            "kw": kw}


def _build():
    out = []
    hurt0 = clicked(0)[1]
    out.append(case("base", hurt0[None, :]))
    # five rows, ragged: full, empty, mid-word, a tile boundary, one sample into the second tile; rows 4-byte but not 16-byte aligned
    rows = np.stack([clicked(s)[1] for s in (1, 2, 3, 4, 5)])
    wide = np.zeros((5, N_BASE + 3), dtype=np.float32)
    wide[:, :N_BASE] = rows
    out.append(case("ragged five", wide, n=N_BASE, lengths=[N_BASE, 0, 5000, 2 * TILE, TILE + 1]))
    out.append(case("ragged five, no lengths", wide, n=N_BASE))
    # the smallest rows: one sample, less than a word, one tile, a one-sample last tile (p < 1: nothing judged there)
    for n in (1, 63, TILE, TILE + 1):
        h = clicked(0, n=max(n, 400), count=2)[1][:n].copy() if n >= 400 else clicked(0, n=400, count=2, at=[20, 50])[1][:n].copy()
        out.append(case("n = %d" % n, h[None, :], order=8 if n < 400 else 32))
    # a click on the last sample of a tile and on the first of the next, alone and together
    for name, at in (("click at tile end", [TILE - 1]), ("click at tile start", [TILE]), ("clicks across the tile boundary", [TILE - 1, TILE])):
        out.append(case(name, clicked(1, count=len(at), at=at)[1][None, :]))
    # the orders and the guards at both ends
    out.append(case("order 1", hurt0[None, :], order=1))
    out.append(case("order 128", hurt0[None, :], order=128))
    out.append(case("guard 0", hurt0[None, :], guard=0, merge_within=0))
    h = clicked(2, at=[30, 4000, TILE - 1, TILE + 64, N_BASE - 5])[1]
    out.append(case("guard 64", h[None, :], guard=64))
    out.append(case("guard 64 short row", h[None, :], guard=64, lengths=[TILE + 100]))
    # the passes, a floor, and k as an fp32 that is no fp64 literal
    big = clicked(3, scale=400.0)[1]
    for passes in (0, 1, 4):
        out.append(case("huge clicks, passes %d" % passes, big[None, :], passes=passes))
    out.append(case("floor", hurt0[None, :], floor=0.05))
    out.append(case("k 3.3", hurt0[None, :], k=3.3))
    # the run rule: drop single flags, no merging, overflow
    out.append(case("min_len 3 guard 0", hurt0[None, :], guard=0, min_len=3))
    out.append(case("overflow", hurt0[None, :], max_gaps=4))
    # non-finite samples: inside the judged part, in the unjudged head, next to a click
    h = hurt0.copy()
    h[5], h[700], h[701], h[TILE + 9] = np.float32("nan"), np.float32("inf"), np.float32("-inf"), np.float32("nan")
    out.append(case("non-finite", h[None, :]))
    # rows that hold nothing: constant, zeros
    flat = np.zeros((2, 5000), dtype=np.float32)
    flat[0] = 0.25
    out.append(case("constant and zero rows", flat))
    assert len({c["name"] for c in out}) == len(out)
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


# ------------------------------------------------------------------------------------------------------------------------------ a long row
# 257 tiles: each thread of the shared gd_rows_kernel owns two, so E = 2 TILE is a thread edge (tests/gap_detect_common.py pins that launch to
# numpy at this length).  Not part of `all_cases()`: its base signal is a Python loop over a million samples.
LONG_N = 256 * TILE + 1
LONG_LENGTHS = (LONG_N, 255 * TILE + 9)
_LONG = []


def long_clicks():
    """clicks `guard` samples either side of two thread edges (the dilation crosses them), in the last full tile, on the last sample of the
    shorter row and on the last sample"""
    E, g = 2 * TILE, DEFAULTS["guard"]
    return [E - g, E + g, 64 * E - g, 64 * E + g, 255 * TILE + 8, 255 * TILE + 100, 255 * TILE + 2000, LONG_N - 1]


def long_case():
    if not _LONG:
        rows = np.stack([clicked(seed, n=LONG_N, at=long_clicks())[1] for seed in (11, 12)])
        _LONG.append(case("long 256 T + 1", rows, lengths=LONG_LENGTHS))
    return _LONG[0]


def measured_margin():
    """4 x the largest relative difference of q / threshold between the two restatements over the judged samples of the table, and the number
    of judged samples compared"""
    worst, seen = 0.0, 0
    for c in all_cases():
        for (_, _, judged, r1), (_, _, _, r2) in zip(masks(c, exact=True), masks(c, exact=False)):
            ok = judged & np.isfinite(r1) & np.isfinite(r2) & (r1 > 0)
            if ok.any():
                worst = max(worst, float(np.max(np.abs(r2[ok] - r1[ok]) / r1[ok])))
                seen += int(ok.sum())
    return 4.0 * worst, seen


def call_kwargs(c):
    return dict(lengths=c["lengths"], **c["kw"])


def clip(c):
    return c["wav"][:, :c["n"]]


def snr_db(ref, est, idx):
    r, d = ref[idx].astype(np.float64), ref[idx].astype(np.float64) - est[idx].astype(np.float64)
    return 10.0 * np.log10(np.dot(r, r) / np.dot(d, d))
