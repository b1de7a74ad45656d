"""Janssen's least-squares AR interpolation of include/viai_hip.h ("crackle and short gaps") restated in numpy fp64 -- np.dot sums, a dense G,
np.linalg.solve -- with the cluster rule in pure Python, and the cases tests/test_janssen_cpu.py and tests/test_janssen_gpu.py share.

The restatement does NOT reproduce the rule's summation orders nor its banded L D L^T: it is a second opinion on the method, not a copy of
the kernel.  The host mirror `janssen_fill_host` is compared with it under a measured tolerance; the device is compared with the host mirror
bit for bit.

    front_k     max(0, start[j] + max(length[j], 0) over j < k): for lists in position order the end of entry k - 1
    usable      1 <= L <= max_len, s >= front_k, s + L <= len; every other entry is skipped (filled 0, nothing written) but still a wall
    clusters    a usable entry joins the open cluster iff s - e_last < context, M + L <= 1024, (M + L)(order + 1) <= 8192 and
                (e - s_first) + 2 context <= 4096; otherwise it opens the next one
    window      [max(s_first - context, front_first, 0), max(min(e_last + context, start of the entry behind, len), e_last))
    iterate     unknowns start at 0; p = min(order, W // 2), p < 1: zeros, code 4; per round: a = burg(window with estimates), b = autocorrelation
                of a, G_ij = b[|t_i - t_j|] within p, r_i = -sum_l b[|l|] x0[t_i + l] over the known samples of the window, x = solve(G, r)

A case is a dict: name, wav (B, stride) float32 with the clip in its first n columns, n, lengths (or None), gaps (count, start, length), the
keyword arguments order / context / iters / max_len, and `noiseless`.  Signals come from `ar_fill_common.tones`."""
import numpy as np

import ar_fill_common as A

MAX_UNKNOWN, BAND_DOUBLES, MAX_WINDOW = 1024, 8192, 4096


def rule_max_len(order, context):
    return min(MAX_UNKNOWN, BAND_DOUBLES // (order + 1), MAX_WINDOW - 2 * context)


# ------------------------------------------------------------------------------------------------------------------------------ the rule
def plan_rule(n, gaps, lengths=None, order=32, context=1024, max_len=None, **_):
    """-> (leader, lo, hi, M), four (B, K) int32 arrays: the cluster rule in plain Python"""
    if max_len is None:
        max_len = rule_max_len(order, context)
    count, start, length = (np.asarray(g) for g in gaps)
    B, K = start.shape
    leader = np.full((B, K), -1, dtype=np.int32)
    lo, hi, unknowns = (np.zeros((B, K), dtype=np.int32) for _ in range(3))
    for b in range(B):
        ln = n if lengths is None else min(max(int(lengths[b]), 0), n)
        listed = min(max(int(count[b]), 0), K)
        ent = [(int(start[b, i]), int(length[b, i])) for i in range(listed)]
        usable, fronts, front = [], [], 0
        for s, L in ent:
            fronts.append(front)
            usable.append(1 <= L <= max_len and s >= front and s + L <= ln)
            front = max(front, s + max(L, 0))
        i = 0
        while i < listed:
            if not usable[i]:
                i += 1
                continue
            s_first, M = ent[i][0], ent[i][1]
            e_last = s_first + M
            j = i + 1
            while j < listed and usable[j]:
                s, L = ent[j]
                if not (s - e_last < context and M + L <= MAX_UNKNOWN and (M + L) * (order + 1) <= BAND_DOUBLES
                        and (s + L - s_first) + 2 * context <= MAX_WINDOW):
                    break
                M, e_last, j = M + L, s + L, j + 1
            w_lo = max(s_first - context, fronts[i], 0)
            w_hi = min(e_last + context, ln)
            if j < listed:
                w_hi = min(w_hi, ent[j][0])
            w_hi = max(w_hi, e_last)
            leader[b, i:j], lo[b, i:j], hi[b, i:j], unknowns[b, i:j] = i, w_lo, w_hi, M
            i = j
    return leader, lo, hi, unknowns


def solve_window(x, t, order, iters):
    """x the window (fp64, known samples finite), t the unknowns' positions -> (estimates, code)"""
    W, M = len(x), len(t)
    p = min(order, W // 2)
    est = np.zeros(M)
    if p < 1:
        return est, 4
    x0 = x.copy()
    x0[t] = 0.0
    xp = np.concatenate((np.zeros(p), x0, np.zeros(p)))
    D = np.abs(t[:, None] - t[None, :])
    for _ in range(iters):
        xx = x0.copy()
        xx[t] = est
        a = A.burg(xx, p)
        b = np.array([np.dot(a[:p + 1 - l], a[l:]) for l in range(p + 1)])
        G = np.where(D <= p, b[np.minimum(D, p)], 0.0)
        both = np.concatenate((b[::-1], b[1:]))
        r = -np.array([np.dot(both, xp[ti:ti + 2 * p + 1]) for ti in t])
        est = np.linalg.solve(G, r)
    return est, 1


def fill_rule(wav, n, gaps, lengths=None, order=32, context=1024, iters=3, max_len=None):
    """-> (out (B, n) float32, filled (B, K) int32)"""
    count, start, length = (np.asarray(g) for g in gaps)
    B, K = start.shape
    leader, lo, hi, _ = plan_rule(n, gaps, lengths, order, context, max_len)
    out = np.array(wav[:, :n], dtype=np.float32, copy=True)
    filled = np.zeros((B, K), dtype=np.int32)
    for b in range(B):
        for k in range(K):
            if leader[b, k] != k:
                continue
            members = [m for m in range(k, K) if leader[b, m] == k]
            w_lo, w_hi = int(lo[b, k]), int(hi[b, k])
            t = np.concatenate([np.arange(int(start[b, m]), int(start[b, m]) + int(length[b, m])) for m in members]) - w_lo
            est, code = solve_window(A.finite64(wav[b, w_lo:w_hi]), t, order, iters)
            with np.errstate(over="ignore"):
                out[b, t + w_lo] = est.astype(np.float32)
            filled[b, members] = code
    return out, filled


_EXPECTED = {}


def expected(case):
    if case["name"] not in _EXPECTED:
        got = fill_rule(case["wav"], case["n"], case["gaps"], case["lengths"], **case["kw"])
        for a in got:
            a.setflags(write=False)
        _EXPECTED[case["name"]] = got
    return _EXPECTED[case["name"]]


def filled_mask(case, filled):
    """(B, n) bool: the samples of the entries whose code is not 0"""
    count, start, length = case["gaps"]
    m = np.zeros((case["wav"].shape[0], case["n"]), dtype=bool)
    for b in range(m.shape[0]):
        for k in range(start.shape[1]):
            if filled[b, k] > 0:
                m[b, start[b, k]:start[b, k] + length[b, k]] = True
    return m


def relative_difference(c, got):
    """max |got - restatement| / the row's peak over the solved samples (the others are compared bit by bit elsewhere)"""
    want, filled = expected(c)
    peak = np.max(np.abs(A.finite64(c["wav"][:, :c["n"]])), axis=1, keepdims=True)
    peak[peak == 0.0] = 1.0
    with np.errstate(invalid="ignore"):
        diff = np.abs(got.astype(np.float64) - want.astype(np.float64)) / peak
    m = filled_mask(c, filled)
    return float(np.max(diff[m])) if m.any() else 0.0


def spans(rows_b):
    return [(s, s + L) for s, L in rows_b]


# ------------------------------------------------------------------------------------------------------------------------------ the cases
CRACKLE_ROWS = [[(1500 + 24 * i, 3) for i in range(40)], [(1500 + 12 * i, 2) for i in range(60)], [(1500 + 40 * i, 5) for i in range(30)]]
SINGLE_ROWS = [[(2000, 64)], [(2000, 160)], [(2000, 240)], [(2000, 16)]]
QUALITY_N = 4200


def crackle_clean(sigma=0.01):
    return A.tones("jn.crackle", 3, QUALITY_N, sigma)


def single_clean(sigma=0.01):
    return A.tones("jn.single", 4, QUALITY_N, sigma)


def case(name, wav, gaps, n=None, lengths=None, noiseless=False, **kw):
    kw.setdefault("order", 32)
    kw.setdefault("context", 1024)
    kw.setdefault("iters", 3)
    kw.setdefault("max_len", None)
    return {"name": name, "wav": wav, "n": wav.shape[1] if n is None else n, "lengths": lengths, "gaps": gaps, "kw": kw, "noiseless": noiseless}


def _build():
    out = []
    tones, damage, lists = A.tones, A.damage, A.lists
    # M = 1: one wild sample (not zeroed: the rule must not read it)
    wav = tones("jn.one", 1, 1500, 0.01)
    wav[0, 700] = 0.9
    out.append(case("one wild sample", wav, lists([[(700, 1)]], 1)))
    # the band's edge: two unknowns exactly p and p + 1 apart
    rows = [[(300, 1), (308, 1)], [(300, 1), (309, 1)]]
    out.append(case("band edge", damage(tones("jn.band", 2, 700, 0.01), rows), lists(rows, 2), order=8, context=64))
    # two runs context - 1 and context apart: joined, not joined
    rows = [[(400, 5), (504, 5)], [(400, 5), (505, 5)]]
    out.append(case("join and no join", damage(tones("jn.join", 2, 1000, 0.01), rows), lists(rows, 2), order=16, context=100))
    # a run that cannot join because of M (order 4: the band would hold 1638), so it opens the next cluster and walls this one
    rows = [[(1500, 600), (2200, 424), (2700, 3)]]
    out.append(case("unknowns limit", damage(tones("jn.m", 1, 4000, 0.01), rows), lists(rows, 3), order=4))
    # ... because of the band (order 32: 248 unknowns)
    rows = [[(1000, 200), (1300, 48), (1400, 1)]]
    out.append(case("band limit", damage(tones("jn.b", 1, 2600, 0.01), rows), lists(rows, 3)))
    # ... because of the window (context 1024: a span of 2048)
    rows = [[(1000 + 500 * i, 2) for i in range(6)]]
    out.append(case("window limit", damage(tones("jn.w", 1, 4700, 0.01), rows), lists(rows, 6), order=8))
    # windows at s = 0 and ending at len
    n = 1200
    rows = [[(0, 10), (40, 3)], [(n - 50, 4), (n - 10, 10)]]
    out.append(case("row ends", damage(tones("jn.ends", 2, n, 0.01), rows), lists(rows, 2), context=256))
    # W = 2 and W = 3 (p = 1) by lengths; W = 1 (no model) by n = 1
    rows = [[(0, 1)], [(1, 1)], [(1, 1)], [(0, 1)]]
    out.append(case("tiny windows", damage(tones("jn.tiny", 4, 8, 0.01), rows), lists(rows, 1), lengths=np.array([2, 2, 3, 1], dtype=np.int32)))
    out.append(case("n = 1", tones("jn.n1", 1, 1, 0.01), lists([[(0, 1)]], 1)))
    # order 1
    rows = [[(500, 20), (530, 7)], [(600, 64)]]
    out.append(case("order 1", damage(tones("jn.o1", 2, 1300, 0.01), rows), lists(rows, 2), order=1, context=512))
    # order 128 with M = 63 and order 7 with M = 1024: both limits met exactly; L = max_len is solved, max_len + 1 is not
    rows = [[(1200, 40), (1300, 23)], [(1200, 63)], [(1200, 64)]]
    out.append(case("order 128", damage(tones("jn.o128", 3, 2600, 0.01), rows), lists(rows, 2), order=128))
    rows = [[(1100, 1024)], [(1100, 1025)], [(1100, 1000), (2200, 24)]]
    out.append(case("order 7", damage(tones("jn.o7", 3, 3300, 0.01), rows), lists(rows, 2), order=7))
    rows = [[(600, 32), (700, 33)]]
    out.append(case("max_len", damage(tones("jn.max", 1, 1500, 0.01), rows), lists(rows, 2), max_len=32, context=512))
    # count > K, count <= 0, an entry out of position order, L <= 0
    rows = [[(300, 6), (340, 6), (380, 6), (420, 6), (460, 6)], [], [(500, 6)], [(400, 5), (700, 0), (720, -3), (300, 5), (-4, 50), (800, 9), (805, 3), (900, 4)]]
    count, start, length = lists(rows, 8)
    start, length = start[:, :8].copy(), length[:, :8].copy()
    count[0], count[2] = 9, -2
    start[0, 5:], length[0, 5:] = 0, 0
    out.append(case("lists that are not lists", damage(tones("jn.lists", 4, 1400, 0.01), [r[:5] if b == 0 else r for b, r in enumerate(rows)]),
                    (count, start, length), context=128, order=12))
    rows3 = [[(300, 6), (340, 6), (380, 6), (420, 6), (460, 6)]]
    c3 = lists(rows3, 3)
    out.append(case("overflow", damage(tones("jn.over", 1, 1400, 0.01), rows3), c3, context=128, order=12))
    # lengths shorter than n in wider rows
    n, stride = 3000, 3011
    rows = [[(900, 20), (960, 12), (2500, 30)]] * 3 + [[(900, 20)]]
    wav = damage(tones("jn.ragged", 4, stride, 0.01), rows)
    out.append(case("ragged rows", wav, lists(rows, 3), n=n, lengths=np.array([2700, 2520, 970, -5], dtype=np.int32)))
    out.append(case("ragged rows, no lengths", wav, lists(rows, 3), n=n))
    # NaN, Inf and -0.0 in a window
    rows = [[(1500, 10), (1530, 4)], [(1500, 30)]]
    wav = damage(tones("jn.nan", 2, 3000, 0.01), rows)
    wav[0, 1400], wav[0, 1520], wav[0, 1700] = np.float32("nan"), np.float32("inf"), np.float32("-inf")
    wav[1, 1499], wav[1, 1600] = np.float32("nan"), np.float32(-0.0)
    out.append(case("non-finite window", wav, lists(rows, 2)))
    # an all-zero window
    out.append(case("all zero", np.zeros((1, 900), dtype=np.float32), lists([[(300, 8), (330, 2)]], 2), context=256))
    # the rows of the quality table
    out.append(case("crackle", damage(crackle_clean(), CRACKLE_ROWS), lists(CRACKLE_ROWS, 64)))
    out.append(case("single gaps", damage(single_clean(), SINGLE_ROWS), lists(SINGLE_ROWS, 1)))
    # one noiseless crackle row: the badly conditioned end of the method
    rows = [CRACKLE_ROWS[0][:20]]
    out.append(case("noiseless crackle", damage(tones("jn.clean", 1, 3600), rows), lists(rows, 20), noiseless=True))
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


def worst_relative_difference(fill, noiseless):
    """max over the noisy (or the noiseless) cases of `relative_difference`; `fill(wav, gaps, lengths=, **kw)` -> (out, filled)"""
    return max(relative_difference(c, fill(c["wav"][:, :c["n"]], c["gaps"], lengths=c["lengths"], **c["kw"])[0])
               for c in all_cases() if c["noiseless"] == noiseless)
