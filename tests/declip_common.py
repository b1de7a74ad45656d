"""Bound-constrained Janssen restoration of include/viai_hip.h ("declipping") restated in numpy fp64 -- np.dot sums, a dense G,
np.linalg.solve -- and the signals and cases tests/test_declip_cpu.py and tests/test_declip_gpu.py share.

The restatement does NOT reproduce the rule's summation orders nor its banded L D L^T: it is a second opinion on the method.  The host mirror
`declip_fill_host` is compared with it under a measured tolerance; the device is compared with the host mirror bit for bit.

    clusters    those of `janssen_fill` (janssen_common.plan_rule)
    window      [max(s_first - context, 0), min(e_last + context, len)), not cut at other entries; read from `src`
    bounds      c = ref at the unknown (non-finite: 0): c > 0 asks x >= c, c < 0 asks x <= c, c == 0 nothing
    iterate     the estimates start at src; per iteration: Burg on the window, the joint solve, then up to `rounds` times: pin every free
                estimate that violates at c, stop if none was pinned or none is free, solve the free ones again with the pinned ones known;
                if rounds >= 1 clamp what still violates
    sweeps      `sweeps` passes over all clusters, pass s reading the result of pass s - 1 (pass 0: the recording), bounds from the recording

A case is a dict: name, wav (B, n) float32, lengths (or None), gaps (count, start, length) and the keyword arguments."""
import math

import numpy as np

import ar_fill_common as A
import janssen_common as J

CLIP = 0.3
SEEDS = (1, 2)


# ------------------------------------------------------------------------------------------------------------------------------ signals
def speechlike(seed, n=2560):
    """-> (clean, clipped), (n,) float32 each: noise plus a pulse every 73 samples through resonances at 500 Hz (r = 0.97) and 1500 Hz
    (r = 0.95) of 16 kHz, peak 1; clipped at +-0.3 inside [256, n - 256) only"""
    rng = np.random.default_rng(seed)
    e = 0.1 * rng.standard_normal(n + 500)
    e[::73] += 1.0
    a = np.array([1.0])
    for r, f in ((0.97, 500.0), (0.95, 1500.0)):
        a = np.convolve(a, [1.0, -2.0 * r * math.cos(2.0 * math.pi * f / 16000.0), r * r])
    y = np.zeros(n + 500)
    for t in range(n + 500):
        acc = e[t]
        for j in range(1, min(t, 4) + 1):
            acc -= a[j] * y[t - j]
        y[t] = acc
    y = y[500:]
    clean = (y / np.max(np.abs(y))).astype(np.float32)
    clipped = clean.copy()
    clipped[256:n - 256] = np.clip(clean[256:n - 256], np.float32(-CLIP), np.float32(CLIP))
    return clean, clipped


_SPEECH = {}


def speech_case(seed):
    """-> dict(clean (1, n), wav (1, n) the clipped row, gaps from find_gaps_host(clip=0.3, min_len=1, max_gaps=256)), computed once"""
    if seed not in _SPEECH:
        from viai_amd.gap_detect import find_gaps_host
        clean, clipped = speechlike(seed)
        wav = clipped[None, :].copy()
        gaps = tuple(np.array(g, copy=True) for g in find_gaps_host(wav, clip=CLIP, min_len=1, max_gaps=256))
        for arr in (wav,) + gaps:
            arr.setflags(write=False)
        _SPEECH[seed] = {"clean": clean[None, :], "wav": wav, "gaps": gaps}
    return _SPEECH[seed]


def listed_mask(gaps, shape, filled=None, code=None):
    """(B, n) bool: the samples of the listed entries (with `filled`: of those whose code is `code`, or not 0 when code is None)"""
    count, start, length = gaps
    m = np.zeros(shape, dtype=bool)
    for b in range(shape[0]):
        for k in range(min(max(int(count[b]), 0), start.shape[1])):
            if filled is not None and (filled[b, k] != code if code is not None else filled[b, k] == 0):
                continue
            if length[b, k] > 0:
                m[b, start[b, k]:start[b, k] + length[b, k]] = True
    return m


def clipped_mask(c):
    """(1, n) bool: the samples of a `speech_case` that were clipped: the listed samples inside [256, n - 256).  (The lists come from the whole
    row, so they also hold the peaks of the unclipped head and tail, whose recorded value is the true one.)"""
    m = listed_mask(c["gaps"], c["wav"].shape)
    m[:, :256] = False
    m[:, c["wav"].shape[1] - 256:] = False
    return m


def snr_db(clean, est, mask):
    r = clean[mask].astype(np.float64)
    d = r - est[mask].astype(np.float64)
    return 10.0 * math.log10(np.dot(r, r) / np.dot(d, d))


def violations(wav, out, mask):
    """how many samples of `mask` lie inside their bound, judged in fp32: sign(c) out < |c|"""
    c, x = wav[mask], out[mask]
    return int(np.sum(((c > 0) & ~(x >= c)) | ((c < 0) & ~(x <= c))))


# ------------------------------------------------------------------------------------------------------------------------------ the rule
def violates(c, x):
    return ((c > 0) & ~(x >= c)) | ((c < 0) & ~(x <= c))


def solve_window(xs, c, t, order, iters, rounds):
    """xs the window of src (fp64, finite), c the bounds of the unknowns, t their positions -> (estimates, code)"""
    W, M = len(xs), len(t)
    p = min(order, W // 2)
    est = xs[t].copy()
    if p < 1:
        return est, 4
    x0 = xs.copy()
    x0[t] = 0.0

    def solve(b, idx, known):
        tt = t[idx]
        D = np.abs(tt[:, None] - tt[None, :])
        G = np.where(D <= p, b[np.minimum(D, p)], 0.0)
        xp = np.concatenate((np.zeros(p), known, np.zeros(p)))
        both = np.concatenate((b[::-1], b[1:]))
        r = -np.array([np.dot(both, xp[ti:ti + 2 * p + 1]) for ti in tt])
        return np.linalg.solve(G, r)

    for _ in range(iters):
        xx = x0.copy()
        xx[t] = est
        a = A.burg(xx, p)
        b = np.array([np.dot(a[:p + 1 - l], a[l:]) for l in range(p + 1)])
        x = solve(b, np.arange(M), x0)
        pinned = np.zeros(M, dtype=bool)
        known = x0.copy()
        for _r in range(rounds):
            new = ~pinned & violates(c, x)
            if not new.any():
                break
            pinned |= new
            x[new] = c[new]
            known[t[new]] = c[new]
            free = np.nonzero(~pinned)[0]
            if free.size == 0:
                break
            x[free] = solve(b, free, known)
        if rounds > 0:
            v = violates(c, x)
            x[v] = c[v]
        est = x
    return est, 1


def sweep_rule(ref, src, gaps, lengths=None, order=32, context=256, iters=2, rounds=3, max_len=None):
    """one sweep -> (out (B, n) float32, filled (B, K) int32, out before the rounding to fp32 (B, n) float64)"""
    count, start, length = (np.asarray(g) for g in gaps)
    B, K = start.shape
    n = ref.shape[1]
    leader, _, _, _ = J.plan_rule(n, gaps, lengths, order, context, max_len)
    out = np.array(src, dtype=np.float32, copy=True)
    exact = out.astype(np.float64)
    filled = np.zeros((B, K), dtype=np.int32)
    for b in range(B):
        ln = n if lengths is None else min(max(int(lengths[b]), 0), n)
        for k in range(K):
            if leader[b, k] != k:
                continue
            members = [m for m in range(k, K) if leader[b, m] == k]
            lo = max(int(start[b, k]) - context, 0)
            hi = min(int(start[b, members[-1]]) + int(length[b, members[-1]]) + context, ln)
            t = np.concatenate([np.arange(int(start[b, m]), int(start[b, m]) + int(length[b, m])) for m in members]) - lo
            est, code = solve_window(A.finite64(src[b, lo:hi]), A.finite64(ref[b, lo:hi])[t], t, order, iters, rounds)
            with np.errstate(over="ignore"):
                out[b, t + lo] = est.astype(np.float32)
            exact[b, t + lo] = est
            filled[b, members] = code
    return out, filled, exact


def fill_rule(wav, gaps, lengths=None, sweeps=3, **kw):
    """-> (out float32, filled, exact float64) of `sweeps` sweeps: a sweep reads the fp32 result of the one before, as the rule does; `exact` holds
    the last sweep's estimates before their rounding to fp32"""
    ref = np.ascontiguousarray(wav, dtype=np.float32)
    src = ref
    for _ in range(sweeps):
        src, filled, exact = sweep_rule(ref, src, gaps, lengths, **kw)
    return src, filled, exact


def relative_difference(wav, gaps, got, want_exact, filled):
    """max |got (fp32) - the restatement before rounding (fp64)| / the row's peak over the samples of the entries with a code"""
    m = listed_mask(gaps, wav.shape, filled)
    if not m.any():
        return 0.0
    peak = np.max(np.abs(A.finite64(wav)), axis=1, keepdims=True)
    peak[peak == 0.0] = 1.0
    return float(np.max((np.abs(got.astype(np.float64) - want_exact) / peak)[m]))


# ------------------------------------------------------------------------------------------------------------------------------ the cases
def clip_rows(clean, rows, level=None):
    """a copy of `clean` with every listed [s, s + L) of every row replaced by +-level with the sign of the clean sample (level None: by the
    smallest magnitude of the run, so that every clean sample of the run satisfies its bound)"""
    hurt = clean.copy()
    for b, r in enumerate(rows):
        for s, L in r:
            seg = clean[b, s:s + L]
            lv = np.float32(np.min(np.abs(seg)) if level is None else level)
            hurt[b, s:s + L] = np.where(seg < 0, -lv, lv).astype(np.float32)
    return hurt


def case(name, wav, gaps, lengths=None, **kw):
    kw.setdefault("order", 32)
    kw.setdefault("context", 256)
    kw.setdefault("iters", 2)
    kw.setdefault("rounds", 3)
    kw.setdefault("sweeps", 1)
    kw.setdefault("max_len", None)
    return {"name": name, "wav": wav, "lengths": lengths, "gaps": gaps, "kw": kw}


def mixed_case():
    """one cluster: a 40-sample run of zeros (a dropout: free) and two clip runs"""
    clean = A.tones("dc.mixed", 1, 1400, 0.01)
    rows = [[(500, 40), (600, 9), (660, 12)]]
    wav = clip_rows(clean, [rows[0][1:]])
    wav[0, 500:540] = 0.0
    return clean, case("mixed list", wav, A.lists(rows, 3), order=16)


def _build():
    out = []
    tones, lists = A.tones, A.lists
    # M = 1
    clean = tones("dc.one", 1, 900, 0.01)
    rows = [[(400, 1)]]
    out.append(case("M = 1", clip_rows(clean, rows), lists(rows, 1)))
    # one run whose every sample violates: the recorded level lies far beyond anything the model predicts -> zero free unknowns, no second solve
    clean = tones("dc.all", 1, 900, 0.01)
    wav = clean.copy()
    wav[0, 400:420] = np.float32(5.0)
    out.append(case("every sample violates", wav, lists([[(400, 20)]], 1)))
    # M = 300 in one cluster at order 16: the compaction crosses the 256-thread stride and all four waves
    clean = tones("dc.m300", 1, 2600, 0.01)
    rows = [[(700 + 20 * i, 6) for i in range(50)]]
    out.append(case("M = 300 at order 16", clip_rows(clean, rows, 0.12), lists(rows, 50), order=16))
    # order 80: the back substitution's second row of lanes, over the compacted set as well
    clean = tones("dc.o80", 1, 2200, 0.01)
    rows = [[(800 + 30 * i, 10) for i in range(10)]]
    out.append(case("order 80", clip_rows(clean, rows, 0.12), lists(rows, 10), order=80))
    # a window clipped at both row ends, lengths shorter than n
    clean = tones("dc.ends", 2, 700, 0.01)
    rows = [[(100, 8), (330, 8)], [(60, 5), (200, 30)]]
    out.append(case("both row ends", clip_rows(clean, rows, 0.1), lists(rows, 2), lengths=np.array([420, 231], dtype=np.int32)))
    # K larger than count, and entries behind count that must not be read
    clean = tones("dc.k", 2, 1000, 0.01)
    rows = [[(300, 6), (340, 6)], [(500, 9)]]
    count, start, length = lists(rows, 5)
    start[:, 3], length[:, 3] = 700, 4
    out.append(case("K larger than count", clip_rows(clean, rows, 0.1), (count, start, length)))
    # an all-zero window: every bound is 0 (free), the fit is a = [1, 0, ...], G the identity: solved, zeros
    out.append(case("all zero", np.zeros((1, 900), dtype=np.float32), lists([[(300, 8), (330, 2)]], 2)))
    # no model: a window of one sample (code 4, the start value is written)
    out.append(case("no model", np.full((1, 1), 0.25, dtype=np.float32), lists([[(0, 1)]], 1)))
    # the badly conditioned end: a noiseless sinusoid and one run of 200.  (No input was found that stops at a pivot: the fit's fp32 inputs
    # keep G positive definite to working precision; the stop is the same code path as janssen_fill's.)
    n = 1500
    wav = (0.5 * np.sin(2.0 * np.pi * 0.01 * np.arange(n)))[None, :].astype(np.float32)
    rows = [[(600, 200)]]
    out.append(case("noiseless sinusoid", clip_rows(wav, rows, 0.05), lists(rows, 1)))
    out.append(clean_mixed()[1])
    assert len({c["name"] for c in out}) == len(out)
    return out


_MIXED = []


def clean_mixed():
    if not _MIXED:
        _MIXED.extend(mixed_case())
    return _MIXED


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
# 257 tiles of `find_gaps` (T = 4096), two per thread of its row launch: the speech-like signal repeated at a quarter of its level, so under
# the clip level, except in two stretches where it is at full level and clipped: one over the thread edge 2 T, one that ends with the row,
# in whose one-sample last tile the signal's largest peak lies.
LONG_T = 4096
LONG_N = 256 * LONG_T + 1
LONG_MAX_GAPS = 256
LONG_STRETCHES = ((2 * LONG_T - 300, 2 * LONG_T + 300), (LONG_N - 400, LONG_N))
_LONG = []


def long_row():
    """(1, LONG_N) float32"""
    if not _LONG:
        clean = speechlike(7)[0]
        top = int(np.argmax(np.abs(clean)))
        assert top >= 400 and abs(float(clean[top])) == 1.0
        wav = (np.tile(clean, -(-LONG_N // clean.size))[:LONG_N] * np.float32(0.25)).astype(np.float32)
        (s0, e0), (s1, e1) = LONG_STRETCHES
        wav[s0:e0] = np.clip(clean[600:600 + e0 - s0], np.float32(-CLIP), np.float32(CLIP))
        wav[s1:e1] = np.clip(clean[top + 1 - (e1 - s1):top + 1], np.float32(-CLIP), np.float32(CLIP))
        wav = wav[None, :].copy()
        wav.setflags(write=False)
        _LONG.append(wav)
    return _LONG[0]


_HOST = {}


def host(c):
    """`declip_fill_host` of a case, computed once and shared"""
    from viai_amd.declip import declip_fill_host
    if c["name"] not in _HOST:
        got = declip_fill_host(c["wav"], c["gaps"], lengths=c["lengths"], **c["kw"])
        for a in got:
            a.setflags(write=False)
        _HOST[c["name"]] = got
    return _HOST[c["name"]]


def tolerance_inputs():
    """(wav, gaps, lengths, kw) of everything the host mirror is compared with the restatement on: the speech-like rows at 1 and 3 sweeps and the
    case table"""
    work = []
    for seed in SEEDS:
        c = speech_case(seed)
        for sweeps in (1, 3):
            work.append((c["wav"], c["gaps"], None, dict(order=32, context=256, iters=2, rounds=3, sweeps=sweeps, max_len=None)))
    work.extend((c["wav"], c["gaps"], c["lengths"], c["kw"]) for c in all_cases())
    return work


def worst_relative_difference(fill):
    """max over `tolerance_inputs` of `relative_difference`; `fill(wav, gaps, lengths=, **kw)` -> (out, filled).  The codes must agree."""
    worst = 0.0
    for wav, gaps, lengths, kw in tolerance_inputs():
        got, filled = fill(wav, gaps, lengths=lengths, **kw)
        _, want_filled, exact = fill_rule(wav, gaps, lengths, **kw)
        assert np.array_equal(filled, want_filled), (filled, want_filled)
        worst = max(worst, relative_difference(wav, gaps, got, exact, filled))
    return worst
