"""CPU: Janssen's least-squares AR interpolation (include/viai_hip.h "crackle and short gaps", csrc/viai_janssen_rule.h) without
a device.  The host mirrors `janssen_fill_host` / `janssen_plan_host` (plain C++ from the rule header the kernel uses) against the numpy
restatement and the pure-Python cluster rule of tests/janssen_common.py; quality against `ar_fill_host` on the same lists; the invariants and
the refusals.

Tolerances.
  fill     max |mirror - restatement| / the row's peak over the solved samples: profiles/janssen_fill_rate.json holds under `tolerance` the
           worst case measured over the sigma = 0.01 cases (`measured`) and ten times that (`allowed`), and the same pair for the noiseless
           row; `allowed` is what is asserted.  The measured figures are 0.0: the two differ by summation order and by L D L^T against LU, a
           few fp64 units, and after the single rounding to fp32 every bit of every solved sample agreed.
  quality  set by the method's purpose, not measured from the code: on crackle Janssen beats the Burg cross-fade by at least 3 dB per row, on
           single gaps it is at most 1 dB below.  Measured at iters = 3: +9.5, +13.0, +4.6 dB and -0.2, +2.6, +3.2, -0.4 dB."""
import json
import os

import numpy as np
import pytest
import torch

import ar_fill_common as A
import janssen_common as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1                                                               # hipErrorInvalidValue


@pytest.fixture(scope="module")
def lib():
    from viai_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def host(c, **over):
    from viai_amd.janssen import janssen_fill_host
    kw = dict(c["kw"])
    kw.update(over)
    return janssen_fill_host(c["wav"][:, :c["n"]], c["gaps"], lengths=c["lengths"], **kw)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def profile():
    with open(os.path.join(ROOT, "profiles", "janssen_fill_rate.json")) as f:
        return json.load(f)


def allowed(noiseless):
    tol = profile()["tolerance"]
    m, a = ("noiseless_measured", "noiseless_allowed") if noiseless else ("measured", "allowed")
    assert tol[a] == pytest.approx(10.0 * tol[m]) and 0.0 <= tol[a] < 1e-5
    return tol[a]


# ----------------------------------------------------------------------------- 1. the cluster rule
@pytest.mark.parametrize("name", J.case_names())
def test_plan_host_equals_the_python_cluster_rule(lib, name):
    from viai_amd.janssen import janssen_plan_host
    c = J.case_by_name(name)
    kw = {k: v for k, v in c["kw"].items() if k != "iters"}
    got = janssen_plan_host(c["n"], c["gaps"], lengths=c["lengths"], **kw)
    want = J.plan_rule(c["n"], c["gaps"], c["lengths"], **kw)
    for g, w, what in zip(got, want, ("leader", "lo", "hi", "M")):
        assert g.dtype == np.int32 and np.array_equal(g, w), (what, g, w)


def test_the_cases_say_what_their_names_say(lib):
    from viai_amd.janssen import janssen_plan_host

    def plan(name):
        c = J.case_by_name(name)
        kw = {k: v for k, v in c["kw"].items() if k != "iters"}
        return [a.tolist() for a in janssen_plan_host(c["n"], c["gaps"], lengths=c["lengths"], **kw)]
    f = lambda name: host(J.case_by_name(name))[1].tolist()
    assert plan("join and no join")[0] == [[0, 0], [0, 1]]                # context - 1 apart: one cluster; context apart: two
    leader, lo, hi, M = plan("unknowns limit")
    assert leader == [[0, 0, 2]] and M == [[1024, 1024, 3]] and hi[0][0] == 2700 and lo[0][2] == 2624   # each is the other's wall
    leader, lo, hi, M = plan("band limit")
    assert leader == [[0, 0, 2]] and M == [[248, 248, 1]] and hi[0][0] == 1400 and lo[0][2] == 1348
    leader, lo, hi, M = plan("window limit")
    assert leader == [[0, 0, 0, 0, 0, 5]] and hi[0][0] == 3500 and hi[0][0] - lo[0][0] <= 4096 and lo[0][5] == 3002
    leader, lo, hi, M = plan("row ends")
    assert lo[0][0] == 0 and hi[1][1] == 1200
    assert f("tiny windows") == [[1], [1], [1], [4]] and f("n = 1") == [[4]]
    assert plan("order 128")[3] == [[63, 63], [63, 0], [0, 0]] and f("order 128") == [[1, 1], [1, 0], [0, 0]]
    assert plan("order 7")[3] == [[1024, 0], [0, 0], [1024, 1024]] and f("order 7") == [[1, 0], [0, 0], [1, 1]]
    assert f("max_len") == [[1, 0]]
    assert f("lists that are not lists") == [[1, 1, 1, 1, 1, 0, 0, 0], [0] * 8, [0] * 8, [1, 0, 0, 0, 0, 1, 0, 1]]
    assert f("overflow") == [[1, 1, 1]]
    assert f("ragged rows") == [[1, 1, 1], [1, 1, 0], [1, 0, 0], [0, 0, 0]]
    got, _ = host(J.case_by_name("all zero"))
    assert not got.any() and not np.signbit(got).any()


# ----------------------------------------------------------------------------- 2. the fill: the whole table against the restatement
@pytest.mark.parametrize("name", J.case_names())
def test_fill_host_equals_the_restatement(lib, name):
    c = J.case_by_name(name)
    got, filled = host(c)
    want, want_filled = J.expected(c)
    assert got.dtype == np.float32 and got.shape == want.shape and filled.dtype == np.int32
    assert np.array_equal(filled, want_filled), (filled, want_filled)
    diff = J.relative_difference(c, got)
    print("%s: max |mirror - restatement| / peak = %.3e" % (name, diff))
    assert diff <= allowed(c["noiseless"])
    m = J.filled_mask(c, want_filled)
    assert np.array_equal(bits(got)[~m], bits(c["wav"][:, :c["n"]])[~m])  # 4a. everything outside the usable runs keeps its bits
    # 4d. skipped entries get 0, the members of one cluster the same code
    kw = {k: v for k, v in c["kw"].items() if k != "iters"}
    leader = J.plan_rule(c["n"], c["gaps"], c["lengths"], **kw)[0]
    assert np.array_equal(filled == 0, leader < 0)
    for b, k in zip(*np.nonzero(leader >= 0)):
        assert filled[b, k] == filled[b, leader[b, k]]


# ----------------------------------------------------------------------------- 3. quality
def test_quality_against_the_burg_cross_fade(lib):
    from viai_amd.ar_fill import ar_fill_host
    from viai_amd.janssen import janssen_fill_host
    recorded = {(r["signal"], r["row"]): r for r in profile()["quality"]}
    for tag, clean, rows, K, margin in (("jn.crackle", J.crackle_clean(), J.CRACKLE_ROWS, 64, 3.0), ("jn.single", J.single_clean(), J.SINGLE_ROWS, 1, -1.0)):
        assert clean.shape[1] == 4200
        hurt, gaps = A.damage(clean, rows), A.lists(rows, K)
        burg, _ = ar_fill_host(hurt, gaps, order=32, context=1024)
        jn, filled = janssen_fill_host(hurt, gaps, order=32, context=1024, iters=3)
        for b, r in enumerate(rows):
            assert (filled[b, :len(r)] == 1).all()
            mine, theirs = A.gap_snr_db(clean[b], jn[b], J.spans(r)), A.gap_snr_db(clean[b], burg[b], J.spans(r))
            print("%s row %d: janssen %.2f dB, burg cross-fade %.2f dB" % (tag, b, mine, theirs))
            assert mine >= theirs + margin, (tag, b, mine, theirs)
            rec = recorded[(tag, b)]
            assert rec["janssen_snr_db_iters3"] == pytest.approx(mine, abs=0.011) and rec["burg_snr_db"] == pytest.approx(theirs, abs=0.011)


# ----------------------------------------------------------------------------- 4. invariants
def test_a_row_alone_is_the_row_in_the_batch_and_twice_is_the_same(lib):
    from viai_amd.janssen import janssen_fill_host
    for name in ("ragged rows", "crackle", "lists that are not lists"):
        c = J.case_by_name(name)
        view = c["wav"][:, :c["n"]]
        whole, filled = host(c)
        again, filled2 = host(c)
        assert np.array_equal(bits(whole), bits(again)) and np.array_equal(filled, filled2)
        for b in range(view.shape[0]):
            ln = None if c["lengths"] is None else c["lengths"][b:b + 1]
            alone, f1 = janssen_fill_host(view[b:b + 1], tuple(g[b:b + 1] for g in c["gaps"]), lengths=ln, **c["kw"])
            assert np.array_equal(bits(alone[0]), bits(whole[b])) and np.array_equal(f1[0], filled[b]), (name, b)


def test_what_a_run_holds_does_not_reach_any_fill(lib):
    c = J.case_by_name("join and no join")
    base, _ = host(c)
    count, start, length = c["gaps"]
    for junk in (np.float32("nan"), np.float32(7e30), np.float32(-0.25)):
        wav = c["wav"].copy()
        for b in range(2):
            for k in range(2):
                wav[b, start[b, k]:start[b, k] + length[b, k]] = junk
        c2 = dict(c, wav=wav)
        got, _ = host(c2)
        m = J.filled_mask(c, np.ones_like(start))
        assert np.array_equal(bits(got)[m], bits(base)[m])


def test_python_entry_points_check_their_arguments(lib):
    from viai_amd import ar_fill, click_detect, gap_detect
    from viai_amd import janssen as M
    from viai_amd._lib import ViaiLibraryError
    assert ar_fill.janssen_fill is M.janssen_fill and ar_fill.janssen_fill_host is M.janssen_fill_host
    assert M.rule_max_len(32, 1024) == 248 and M.rule_max_len(7, 1024) == 1024 and M.rule_max_len(128, 1024) == 63 and M.rule_max_len(1, 1024) == 1024
    assert M.rule_max_len(1, 1800) == 496
    wav = np.zeros((1, 64), dtype=np.float32)
    gaps = A.lists([[(10, 5)]], 1)
    tg = tuple(torch.from_numpy(g) for g in gaps)
    with pytest.raises(ViaiLibraryError):
        M.janssen_fill(torch.zeros(1, 64), tg)                            # a CPU tensor: no fallback
    for bad in (dict(order=0), dict(order=129), dict(context=1), dict(context=1025), dict(iters=0), dict(iters=17), dict(max_len=0),
                dict(max_len=249), dict(order=7, max_len=1025), dict(order=128, max_len=64), dict(order=1.5), dict(iters=2.5)):
        with pytest.raises(ValueError):
            M.janssen_fill_host(wav, gaps, **bad)
        with pytest.raises(ValueError):
            M.janssen_fill(torch.zeros(1, 64), tg, **bad)                 # before the device is asked for
    for ok in (dict(max_len=248), dict(order=7, max_len=1024), dict(order=128, max_len=63), dict(iters=16), dict(context=2)):
        M.janssen_fill_host(wav, gaps, **ok)
    with pytest.raises(ValueError):
        M.janssen_fill_host(np.zeros(64, dtype=np.float32), gaps)
    with pytest.raises(ValueError):
        M.janssen_fill_host(wav, gaps, lengths=[1, 2])
    with pytest.raises(ValueError):
        M.janssen_plan_host(0, gaps)
    for bad in (dict(method="lpc"), dict(ar_iters=2), dict(method="janssen", ar_iters=0)):
        with pytest.raises(ValueError):
            click_detect.declick_host(wav, **bad)
    for bad in (dict(ar_method="lpc"), dict(ar_iters=2)):
        with pytest.raises(ValueError):
            gap_detect.repair(None, torch.zeros(1, 64), gaps=tg, ar_below=8, **bad)


def test_every_refusal_is_invalid_value_without_a_device(lib):
    """the pointers are never dereferenced by a refused call: small fake addresses"""
    wav, cnt, st, ln, out, fl = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000

    def args(wav=wav, lengths=None, stride=100, B=2, n=100, count=cnt, start=st, length=ln, K=4, order=32, context=1024, max_len=248, iters=3,
             out=out, out_stride=100, filled=fl):
        return (wav, lengths, stride, B, n, count, start, length, K, order, context, max_len, iters, out, out_stride, filled)
    bad = [dict(wav=None), dict(count=None), dict(start=None), dict(length=None), dict(out=None), dict(filled=None), dict(B=0), dict(K=0),
           dict(n=0), dict(n=1 << 31, stride=1 << 31, out_stride=1 << 31), dict(stride=99), dict(out_stride=99), dict(order=0), dict(order=129),
           dict(context=1), dict(context=1025), dict(max_len=0), dict(max_len=249), dict(iters=0), dict(iters=17), dict(B=1 << 16, K=1 << 15)]
    for kw in bad:
        assert lib.viai_janssen_fill(*args(**kw), None) == INVALID, kw
        assert lib.viai_janssen_fill_host(*args(**kw)) == INVALID, kw
    assert lib.viai_janssen_fill(*args(wav=0x1002), None) == INVALID      # the device call wants 4-byte aligned rows
    assert lib.viai_janssen_plan_host(None, 1, 100, cnt, st, ln, 4, 32, 1024, 249, 0x7000, 0x7100, 0x7200, 0x7300) == INVALID
    assert lib.viai_janssen_plan_host(None, 1, 100, cnt, st, ln, 4, 32, 1024, 248, None, 0x7100, 0x7200, 0x7300) == INVALID


# ----------------------------------------------------------------------------- 5. the pass-throughs
def crackled():
    """a crackle row `find_clicks_host` lists in full with its defaults: 20 wild samples, one every 48"""
    clean = J.crackle_clean()[:1].copy()
    hurt = clean.copy()
    pos = np.arange(1500, 1500 + 48 * 20, 48)
    hurt[0, pos] += np.where(np.arange(20) % 2 == 0, 0.5, -0.5).astype(np.float32)
    return clean, hurt, pos


def test_declick_host_janssen_is_find_clicks_then_janssen_fill(lib):
    from viai_amd.click_detect import declick_host, find_clicks_host
    from viai_amd.janssen import janssen_fill_host
    clean, hurt, pos = crackled()
    out, gaps, filled = declick_host(hurt, method="janssen", ar_iters=2)
    g2 = find_clicks_host(hurt)
    want, f2 = janssen_fill_host(hurt, g2, order=32, context=1024, iters=2)
    assert 20 <= int(gaps.count[0]) <= 64 and (filled[0, :int(gaps.count[0])] == 1).all() and all(np.array_equal(a, b) for a, b in zip(gaps, g2))
    assert np.array_equal(bits(out), bits(want)) and np.array_equal(filled, f2)
    out3, _, _ = declick_host(hurt, method="janssen")                     # ar_iters defaults to janssen_fill's 3
    assert np.array_equal(bits(out3), bits(janssen_fill_host(hurt, g2)[0]))


def test_the_defaults_are_the_burg_path_bit_for_bit(lib):
    from viai_amd.ar_fill import ar_fill_host
    from viai_amd.click_detect import declick_host, find_clicks_host
    clean, hurt, pos = crackled()
    out, gaps, filled = declick_host(hurt)
    same, _, f2 = declick_host(hurt, method="burg")
    want, f3 = ar_fill_host(hurt, find_clicks_host(hurt), order=32, context=1024)
    assert np.array_equal(bits(out), bits(want)) and np.array_equal(bits(same), bits(want))
    assert np.array_equal(filled, f3) and np.array_equal(f2, f3)
    import inspect

    from viai_amd import gap_detect, wav_io
    for fn in (gap_detect.repair, wav_io.repair_file):
        sig = inspect.signature(fn).parameters
        assert sig["ar_method"].default == "burg" and sig["ar_iters"].default is None and sig["ar_below"].default == 0
