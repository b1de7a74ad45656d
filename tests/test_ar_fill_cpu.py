"""CPU: the autoregressive gap fill (include/viai_hip.h "short gaps", csrc/viai_ar_rule.h) without a device.  The host mirror
`ar_fill_host` / `ar_fit_host` (plain C++ from the rule header the kernel uses) against the numpy fp64 restatement of tests/ar_fill_common.py,
which sums with np.dot and so differs from the mirror by summation order only; the exact cases, the edges, the untouched bits, and the refusals.

Tolerances.
  fill   max |mirror - restatement| / the row's peak over the filled samples: profiles/ar_fill_rate.json holds under `tolerance` the worst case
         measured over the case table (`worst`) and ten times that (`allowed`), which is what is asserted here.
  fit    |a - a_restated| <= 1e-7 max(1, max |a|).  Reasoning, not a measurement: a dot product of C <= 4096 fp64 terms is off by at most
         C eps = 4.5e-13 of the sum of its terms' magnitudes; a reflection coefficient divides by the residual power, which the sigma = 0.01
         noise keeps above 1e-4 against a signal power of 0.06 (a factor 600); 128 stages add up: 4.5e-13 x 600 x 128 = 3.5e-8."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import ar_fill_common as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1                                                               # hipErrorInvalidValue


@pytest.fixture(scope="module")
def lib():
    from viai_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def host(c, **over):
    from viai_amd.ar_fill import ar_fill_host
    kw = dict(c["kw"])
    kw.update(over)
    return ar_fill_host(c["wav"][:, :c["n"]], c["gaps"], lengths=c["lengths"], **kw)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def allowed():
    with open(os.path.join(ROOT, "profiles", "ar_fill_rate.json")) as f:
        tol = json.load(f)["tolerance"]
    assert tol["allowed"] == pytest.approx(10.0 * tol["worst"]) and 0.0 < tol["allowed"] < 1e-5
    return tol["allowed"]


# ----------------------------------------------------------------------------- 1. the fit
@pytest.mark.parametrize("order", (1, 2, 31, 32, 128))
def test_fit_host_equals_the_restatement(lib, order):
    from viai_amd.ar_fill import ar_fit_host
    x = A.tones("ar.fit", 1, 4096, 0.01)[0]
    for n in (2, 3, 255, 256, 257, 1024, 4096):                           # either side of the 256-partial stride, and the limits
        a, p = ar_fit_host(x[:n], order)
        assert p == min(order, n // 2) and a.shape == (order + 1,) and a.dtype == np.float64
        want = A.burg(x[:n], p)
        assert a[0] == 1.0 and not a[p + 1:].any()
        assert np.max(np.abs(a[:p + 1] - want)) <= 1e-7 * max(1.0, np.max(np.abs(want))), (order, n)
    a, p = ar_fit_host(x[:0], order)                                      # no sample at all: the identity model
    assert p == 0 and a[0] == 1.0 and not a[1:].any()


# ----------------------------------------------------------------------------- 2. the fill: the whole table against the restatement
@pytest.mark.parametrize("name", A.case_names())
def test_fill_host_equals_the_restatement(lib, name):
    c = A.case_by_name(name)
    got, filled = host(c)
    want, want_filled = A.expected(c)
    assert got.dtype == np.float32 and got.shape == want.shape and filled.dtype == np.int32
    assert np.array_equal(filled, want_filled), (filled, want_filled)
    diff = A.relative_difference(c, got)
    print("%s: max |mirror - restatement| / peak = %.3e" % (name, diff))
    assert diff <= allowed()
    m = A.filled_mask(c, want_filled)
    assert np.array_equal(bits(got)[~m], bits(c["wav"][:, :c["n"]])[~m])  # everything else keeps its bits


def test_the_cases_say_what_their_names_say(lib):
    f = lambda name: A.expected(A.case_by_name(name))[1].tolist()
    assert f("row ends") == [[3, 0], [2, 0], [4, 0], [3, 2]]              # at 0; at len; the whole row; one context sample on a side
    assert f("ragged rows") == [[1, 1], [1, 0], [1, 0], [0, 0]]           # the gap that crosses len and the one behind it are skipped
    assert f("neighbours") == [[1, 1, 0], [2, 4, 3], [0, 1, 1]]           # touching gaps have no context between them
    assert f("max_len and no gaps") == [[1, 0, 0, 0], [0, 0, 0, 1]]
    assert f("overflow and empty") == [[1, 1, 1], [0, 0, 0], [0, 0, 0]]
    c = A.case_by_name("row ends")
    got, _ = host(c)
    assert not got[2].any()                                               # a row that is one gap: zeros


# ----------------------------------------------------------------------------- 3. quality
QUALITY_HZ = (313.0, 1777.0, 3511.0)


def test_quality_floor_on_noiseless_tones(lib):
    from viai_amd.ar_fill import ar_fill_host
    n, L = 4000, 160
    wav = A.tones("ar.q", 4, n, 0.0, freqs=[QUALITY_HZ] * 4)
    rows = [[(1500 + 37 * b, L)] for b in range(4)]
    hurt, gaps = A.damage(wav, rows), A.lists(rows, 1)
    got, filled = ar_fill_host(hurt, gaps, order=32, context=1024)
    want, _ = A.fill_rule(hurt, n, gaps, order=32, context=1024)
    assert filled.tolist() == [[1]] * 4
    for b in range(4):
        span = [(rows[b][0][0], rows[b][0][0] + L)]
        mine, ref = A.gap_snr_db(wav[b], got[b], span), A.gap_snr_db(wav[b], want[b], span)
        print("row %d: gap SNR %.1f dB, restatement %.1f dB" % (b, mine, ref))
        assert ref >= 60.0 and mine >= 40.0 and abs(mine - ref) <= 1.0


# ----------------------------------------------------------------------------- 4. exact cases
def test_dc_and_zero_contexts_are_exact(lib):
    from viai_amd.ar_fill import ar_fill_host, ar_fit_host
    n = 1500
    for value in (0.375, -0.1, 1e-20):
        wav = np.full((1, n), value, dtype=np.float32)
        rows = [[(600, 100), (1000, 64)]]
        got, filled = ar_fill_host(A.damage(wav, rows), A.lists(rows, 2), order=8, context=256)
        assert filled.tolist() == [[1, 1]] and np.array_equal(bits(got), bits(wav)), value    # k = -1, then denominator 0: a = [1, -1, 0, ...]
        a, p = ar_fit_host(wav[0, :300], 8)
        assert p == 8 and a.tolist() == [1.0, -1.0] + [0.0] * 7
    zeros = np.zeros((1, n), dtype=np.float32)
    got, filled = ar_fill_host(zeros, A.lists([[(600, 100)]], 1))
    assert filled.tolist() == [[1]] and not got.any() and not np.signbit(got).any()


# ----------------------------------------------------------------------------- 5. neighbours and untouched bits
def test_a_neighbours_content_does_not_reach_a_fill(lib):
    from viai_amd.ar_fill import ar_fill_host
    c = A.case_by_name("neighbours")
    base, _ = host(c)
    count, start, length = c["gaps"]
    for junk in (np.float32("nan"), np.float32(7e30), np.float32(-0.25)):
        wav = c["wav"].copy()
        s, L = int(start[0, 1]), int(length[0, 1])
        wav[0, s:s + L] = junk                                            # inside gap 1 of row 0, 10 samples behind gap 0
        got, _ = ar_fill_host(wav, c["gaps"], **c["kw"])
        s0, L0 = int(start[0, 0]), int(length[0, 0])
        assert np.array_equal(bits(got[0, s0:s0 + L0]), bits(base[0, s0:s0 + L0]))
        assert np.array_equal(bits(got[0, s:s + L]), bits(base[0, s:s + L]))          # and its own fill does not read what it replaces


def test_untouched_samples_keep_their_bits(lib):
    from viai_amd.ar_fill import ar_fill_host
    c = A.case_by_name("max_len and no gaps")
    wav = c["wav"].copy()
    raw = wav.view(np.int32)
    raw[0, 10], raw[0, 1499], raw[0, 1629] = 0x7fc12345, -0x800000 + 0x77, -0x80000000      # NaN payloads and -0.0: in a context, at a skipped gap's edges
    wav[1, 5] = np.float32("inf")
    got, filled = ar_fill_host(wav, c["gaps"], **c["kw"])
    assert filled.tolist() == [[1, 0, 0, 0], [0, 0, 0, 1]]
    m = A.filled_mask(c, filled)
    assert np.array_equal(bits(got)[~m], raw[~m]) and m.sum() == 128 + 64
    assert np.array_equal(bits(got[0, 1500:1629]), raw[0, 1500:1629])     # the gap longer than max_len is as it was
    # count = 0 everywhere: nothing is touched
    count, start, length = c["gaps"]
    got, filled = ar_fill_host(wav, (np.zeros_like(count), start, length), **c["kw"])
    assert not filled.any() and np.array_equal(bits(got), raw)
    # count > K fills the first K only
    c = A.case_by_name("overflow and empty")
    got, filled = host(c)
    assert int(c["gaps"][0][0]) == 5 and filled[0].tolist() == [1, 1, 1]
    assert np.array_equal(bits(got[0, 1400:]), bits(c["wav"][0, 1400:]))  # gaps 3 and 4 of the row are not in the lists


def test_a_row_alone_is_the_row_in_the_batch_and_strided_rows_are_read_in_place(lib):
    from viai_amd.ar_fill import ar_fill_host
    c = A.case_by_name("ragged rows")
    n = c["n"]
    view = c["wav"][:, :n]
    assert view.strides[0] > 4 * n                                        # a view of wider rows
    whole, filled = ar_fill_host(view, c["gaps"], lengths=c["lengths"], **c["kw"])
    packed, filled2 = ar_fill_host(np.ascontiguousarray(view), c["gaps"], lengths=c["lengths"], **c["kw"])
    assert np.array_equal(bits(whole), bits(packed)) and np.array_equal(filled, filled2)
    for b in range(view.shape[0]):
        alone, f1 = ar_fill_host(view[b:b + 1], tuple(g[b:b + 1] for g in c["gaps"]), lengths=c["lengths"][b:b + 1], **c["kw"])
        assert np.array_equal(bits(alone[0]), bits(whole[b])) and np.array_equal(f1[0], filled[b]), b


# ----------------------------------------------------------------------------- 6. refusals
def test_python_entry_points_check_their_arguments(lib):
    from viai_amd import ar_fill as M
    from viai_amd._lib import ViaiLibraryError
    wav = np.zeros((1, 64), dtype=np.float32)
    gaps = A.lists([[(10, 5)]], 1)
    tg = tuple(torch.from_numpy(g) for g in gaps)
    with pytest.raises(ViaiLibraryError):
        M.ar_fill(torch.zeros(1, 64), tg)                                 # a CPU tensor: no fallback
    for bad in (dict(order=0), dict(order=129), dict(context=1), dict(context=4097), dict(max_len=0), dict(max_len=4097), dict(order=1.5)):
        with pytest.raises(ValueError):
            M.ar_fill_host(wav, gaps, **bad)
        with pytest.raises(ValueError):
            M.ar_fill(torch.zeros(1, 64), tg, **bad)
    with pytest.raises(ValueError):
        M.ar_fill_host(np.zeros(64, dtype=np.float32), gaps)
    with pytest.raises(ValueError):
        M.ar_fill_host(wav, (gaps[0], gaps[1], gaps[2][:, :0]))
    with pytest.raises(ValueError):
        M.ar_fill_host(wav, gaps, lengths=[1, 2])
    with pytest.raises(ValueError):
        M.ar_fit_host(np.zeros(8, dtype=np.float32), 0)
    with pytest.raises(ValueError):
        M.ar_fit_host(np.zeros(4097, dtype=np.float32), 4)
    from viai_amd import gap_detect
    with pytest.raises(ValueError):
        gap_detect.repair(None, torch.zeros(1, 64), gaps=tg, ar_below=-1)


def test_every_refusal_is_invalid_value_without_a_device(lib):
    """the pointers are never dereferenced by a refused call: small fake addresses"""
    wav, cnt, st, ln, out, fl = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000

    def args(wav=wav, lengths=None, stride=100, B=2, n=100, count=cnt, start=st, length=ln, K=4, order=32, context=1024, max_len=4096, out=out,
             out_stride=100, filled=fl):
        return (wav, lengths, stride, B, n, count, start, length, K, order, context, max_len, out, out_stride, filled)
    bad = [dict(wav=None), dict(count=None), dict(start=None), dict(length=None), dict(out=None), dict(filled=None), dict(B=0), dict(B=-1),
           dict(K=0), dict(K=-3), dict(n=0), dict(n=1 << 31, stride=1 << 31, out_stride=1 << 31), dict(stride=99), dict(out_stride=99),
           dict(order=0), dict(order=129), dict(context=1), dict(context=4097), dict(max_len=0), dict(max_len=4097),
           dict(B=1 << 16, K=1 << 15)]
    for kw in bad:
        assert lib.viai_ar_fill(*args(**kw), None) == INVALID, kw
        assert lib.viai_ar_fill_host(*args(**kw)) == INVALID, kw
    assert lib.viai_ar_fill(*args(wav=0x1002), None) == INVALID           # the device call wants 4-byte aligned rows
    a, p = (C.c_double * 9)(), C.c_int()
    x = (C.c_float * 8)()
    for xx, n, order, aa, pp in ((None, 8, 4, a, C.byref(p)), (x, 8, 4, None, C.byref(p)), (x, 8, 4, a, None), (x, -1, 4, a, C.byref(p)),
                                 (x, 4097, 4, a, C.byref(p)), (x, 8, 0, a, C.byref(p)), (x, 8, 129, a, C.byref(p))):
        assert lib.viai_ar_fit_host(xx, n, order, aa, pp) == INVALID
