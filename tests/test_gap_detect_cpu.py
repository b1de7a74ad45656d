"""CPU: the gap-detection rule (include/viai_hip.h) without a device.  The numpy statement of the rule gives lists written out by
hand; `find_gaps_host` (plain C++, sample by sample) equals it exactly on every case the GPU test runs; the workspace size is host arithmetic; and
`viai_gap_detect` refuses bad arguments before any launch, so also here.  The vectorised statement `raw_runs_fast` equals the sample loop on
every row of the table, and with it `find_gaps_host` equals the rule on the long rows of the GPU test (256 T + 1 and 600 T + 5 samples:
test_find_gaps_host_equals_the_numpy_rule_on_long_rows)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import gap_detect_common as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1                                                               # hipErrorInvalidValue


@pytest.fixture(scope="module")
def lib():
    from viai_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_tile_constant_is_the_headers():
    from viai_amd import gap_detect
    text = open(os.path.join(ROOT, "include", "viai_hip.h")).read()
    tile = int(re.search(r"#define\s+VIAI_GAP_DETECT_TILE\s+(\d+)", text).group(1))
    assert tile == G.T == gap_detect.TILE and tile & (tile - 1) == 0 and tile % 64 == 0


# ----------------------------------------------------------------------------- 1. the numpy rule, on lists written out by hand
def lists(got):
    count, start, length = got
    return [int(c) for c in count], [list(map(int, r)) for r in start], [list(map(int, r)) for r in length]


def test_numpy_rule_on_hand_written_cases():
    z = np.float32(0)
    x = np.full((1, 20), 0.5, dtype=np.float32)
    x[0, 2:5] = z                                                         # 3 long
    x[0, 7:12] = z                                                        # 5 long
    x[0, 14:20] = z                                                       # 6 long, ends with the row
    assert lists(G.rule(x, 20, min_len=1, max_gaps=4)) == ([3], [[2, 7, 14, 0]], [[3, 5, 6, 0]])
    assert lists(G.rule(x, 20, min_len=4, max_gaps=4)) == ([2], [[7, 14, 0, 0]], [[5, 6, 0, 0]])
    assert lists(G.rule(x, 20, min_len=7, max_gaps=4)) == ([0], [[0, 0, 0, 0]], [[0, 0, 0, 0]])
    # merging: 7 - 5 = 2 and 14 - 12 = 2
    assert lists(G.rule(x, 20, min_len=1, merge_within=1, max_gaps=4)) == ([3], [[2, 7, 14, 0]], [[3, 5, 6, 0]])
    assert lists(G.rule(x, 20, min_len=1, merge_within=2, max_gaps=4)) == ([1], [[2, 0, 0, 0]], [[18, 0, 0, 0]])
    # the distance is between KEPT runs: with min_len 5 the first run is dropped and the others are 14 - 12 = 2 apart
    assert lists(G.rule(x, 20, min_len=5, merge_within=1, max_gaps=4)) == ([2], [[7, 14, 0, 0]], [[5, 6, 0, 0]])
    assert lists(G.rule(x, 20, min_len=5, merge_within=2, max_gaps=4)) == ([1], [[7, 0, 0, 0]], [[13, 0, 0, 0]])
    # ... and a dropped run between two kept ones counts as ordinary samples: kept [2, 5), dropped [8, 10), kept [14, 20), 14 - 5 = 9
    x[0, 7:12] = 0.5
    x[0, 8:10] = z
    assert lists(G.rule(x, 20, min_len=3, merge_within=8, max_gaps=4)) == ([2], [[2, 14, 0, 0]], [[3, 6, 0, 0]])
    assert lists(G.rule(x, 20, min_len=3, merge_within=9, max_gaps=4)) == ([1], [[2, 0, 0, 0]], [[18, 0, 0, 0]])
    # overflow: the true count, the first K
    assert lists(G.rule(x, 20, min_len=1, max_gaps=2)) == ([3], [[2, 8]], [[3, 2]])
    assert lists(G.rule(x, 20, min_len=1, max_gaps=1)) == ([3], [[2]], [[3]])
    # lengths: a run is cut at len, samples beyond do not exist, out-of-range values are clamped
    y = np.tile(x, (5, 1))
    got = G.rule(y, 20, lengths=[0, 16, 14, 99, -1], min_len=1, max_gaps=3)
    assert lists(got) == ([0, 3, 2, 3, 0], [[0, 0, 0], [2, 8, 14], [2, 8, 0], [2, 8, 14], [0, 0, 0]],
                          [[0, 0, 0], [3, 2, 2], [3, 2, 0], [3, 2, 6], [0, 0, 0]])
    # the predicate
    f = np.float32
    p = np.array([[0.5, np.nan, 0.5, np.inf, 0.5, -np.inf, 0.5, -0.0, 0.5, 1e-40, 0.5, 0.25, 0.5, -1.0, 0.5, 0.75]], dtype=np.float32)
    assert lists(G.rule(p, 16, min_len=1, max_gaps=8))[1] == [[1, 3, 5, 7, 0, 0, 0, 0]]                     # the denormal is a sample
    assert lists(G.rule(p, 16, min_len=1, max_gaps=8, threshold=0.25))[1] == [[1, 3, 5, 7, 9, 11, 0, 0]]
    assert lists(G.rule(p, 16, min_len=1, max_gaps=8, threshold=float(np.nextafter(f(0.25), f(0)))))[1] == [[1, 3, 5, 7, 9, 0, 0, 0]]
    assert lists(G.rule(p, 16, min_len=1, max_gaps=8, clip=0.75))[1] == [[1, 3, 5, 7, 13, 15, 0, 0]]
    assert lists(G.rule(p, 16, min_len=1, max_gaps=8, clip=float(np.nextafter(f(0.75), f(1)))))[1] == [[1, 3, 5, 7, 13, 0, 0, 0]]


def test_the_shared_cases_say_what_their_names_say():
    """the builders place runs where the issue wants them: spot checks against the numpy rule"""
    names = G.case_names()
    for n in G.GEOMETRY_N:
        assert "geometry n=%d min_len=4" % n in names
    count, start, length = G.expected(G.case_by_name("geometry n=%d min_len=4" % (3 * G.T + 17)))
    rows = G.geometry_rows(3 * G.T + 17)
    b = rows.index([(G.T - 3, 3 * G.T + 5)])
    assert (count[b], start[b, 0], length[b, 0]) == (1, G.T - 3, 2 * G.T + 8)
    b = rows.index([(8, 11), (20, 24)])
    assert (count[b], start[b, 0], length[b, 0]) == (1, 20, 4)
    count, start, length = G.expected(G.case_by_name("merging within 10"))
    assert count[0] == 6 and list(start[0, :6]) == [100, 141, 300, 500, 600, 621] and list(length[0, :6]) == [30, 9, 40, 30, 10, 9]
    count, start, length = G.expected(G.case_by_name("overflow K=3"))
    assert list(count) == [10, 9, 1, 0] and list(start[0]) == [0, 40, 100] and list(start[3]) == [0, 0, 0]
    count, start, length = G.expected(G.case_by_name("overflow K=1 merging"))                              # pairs 30 apart join, 50 apart do not
    assert list(count) == [5, 1, 1, 0] and list(start[:, 0]) == [0, G.T - 100, 7, 0] and list(length[:, 0]) == [50, 330, 10, 0]
    count, _, _ = G.expected(G.case_by_name("predicate zeros only"))
    assert count[0] == 5 + 1                                              # NaN, +Inf, -Inf, -0.0, 0.0 and the run at the end
    for p in G.RANDOM_P:
        count, _, _ = G.expected(G.case_by_name("random p=%g min_len=1 merge=0" % p))
        assert count.min() > 64                                           # more runs than the lists hold: the true count is checked


# ----------------------------------------------------------------------------- 2. the host function is the numpy rule
@pytest.mark.parametrize("name", G.case_names())
def test_find_gaps_host_equals_the_numpy_rule(name):
    from viai_amd.gap_detect import find_gaps_host
    c = G.case_by_name(name)
    got = find_gaps_host(c["wav"][:, :c["n"]], lengths=c["lengths"], **c["kw"])
    want = G.expected(c)
    for g, w, what in zip(got, want, ("count", "start", "length")):
        assert g.dtype == np.int32 and g.shape == w.shape and np.array_equal(g, w), what


# ----------------------------------------------------------------------------- 2b. rows of millions of samples (gap_detect_common.long_rows)
def test_the_vectorised_rule_is_the_sample_loop_on_every_row_of_the_table():
    rows = 0
    for c in G.all_cases():
        kw = dict(threshold=0.0, clip=0.0)
        kw.update(c["kw"])
        for b in range(c["wav"].shape[0]):
            ln = c["n"] if c["lengths"] is None else min(max(int(c["lengths"][b]), 0), c["n"])
            assert G.raw_runs_fast(c["wav"][b], ln, kw["threshold"], kw["clip"]) == G.raw_runs(c["wav"][b], ln, kw["threshold"], kw["clip"]), (c["name"], b)
            rows += 1
    assert rows == 311 and len(G.all_cases()) == 56


def test_the_long_cases_say_what_their_names_say():
    """the lengths put more than one tile on a thread of gd_rows_kernel, and the runs lie on the edges the builders name"""
    T = G.T
    for per, n in G.LONG_N.items():
        ntiles = -(-n // T)
        assert -(-ntiles // G.ROWS_THREADS) == per and n % 2 == 1 and n > G.ROWS_THREADS * T
        last_owner, left = (ntiles - 1) // per, ntiles - (ntiles - 1) // per * per
        assert (per, ntiles, last_owner, left, n - (ntiles - 1) * T) in ((2, 257, 128, 1, 1), (3, 601, 200, 1, 5))
        E, tag = per * T, "long per=%d " % per
        count, start, length = G.expected(G.long_case_by_name(tag + "geometry min_len=4"))
        assert list(count) == [1, 1, 1, 1, 1, 0] and list(start[:5, 0]) == [E + T - 3, E - 3, E + T - 5, 0, 100 * T + 9]
        assert list(length[:5, 0]) == [6, 6, 4 * E + 12, n, n - 100 * T - 9]
        count, start, length = G.expected(G.long_case_by_name(tag + "geometry min_len=1"))
        assert (count[5], start[5, 0], length[5, 0]) == (1, n - 1, 1)
        joined, apart = G.expected(G.long_case_by_name(tag + "merging within 6")), G.expected(G.long_case_by_name(tag + "merging within 5"))
        assert list(joined[0]) == [1, 1, 1] and list(apart[0]) == [2, 2, 2]
        assert list(joined[1][:, 0]) == [E - 13, 2 * E - 16, E + T - 13] and list(joined[2][:, 0]) == [26, 28, 26]
        assert list(apart[1][1, :2]) == [2 * E - 16, 2 * E + 2]                      # the dropped run on the edge is not listed
        count, start, length = G.expected(G.long_case_by_name(tag + "overflow K=3"))
        assert list(count) == [10, 10] and start[0, 2] > 2 * 25 * T and list(start[1]) == [3 * E - 5, 15 * E - 5, 27 * E - 5]
        count, start, length = G.expected(G.long_case_by_name(tag + "K=1 merging all"))
        assert list(count) == [1, 1] and list(start[:, 0]) == [100, 3 * E - 5] and list(length[1]) == [108 * E + 10]
        c = G.long_case_by_name(tag + "ragged")
        count, start, length = G.expected(c)
        L = (ntiles - 1) * T
        assert list(c["lengths"]) == [0, E, L + 1, n + 50, -3] and list(count) == [0, 1, 3, 3, 0]
        assert (start[1, 0], length[1, 0]) == (E - 6, 6) and (start[2, 2], length[2, 2]) == (L - 4, 5) and length[3, 2] == n - L + 4
        for p in G.LONG_RANDOM_P:
            count, _, _ = G.expected(G.long_case_by_name(tag + "random p=%g min_len=1 merge=0" % p))
            assert count.min() > 64 * 100                                 # runs in every tile: every thread's loops carry


@pytest.mark.parametrize("name", G.long_case_names())
def test_find_gaps_host_equals_the_numpy_rule_on_long_rows(name):
    from viai_amd.gap_detect import find_gaps_host
    c = G.long_case_by_name(name)
    got = find_gaps_host(c["wav"], lengths=c["lengths"], **c["kw"])
    for g, w, what in zip(got, G.expected(c), ("count", "start", "length")):
        assert g.dtype == np.int32 and g.shape == w.shape and np.array_equal(g, w), what


def test_host_function_overwrites_every_output_entry(lib):
    c = G.case_by_name("overflow K=3")
    wav = np.ascontiguousarray(c["wav"])
    B, n = wav.shape
    for K in (1, 3, 16):
        count = np.full(B, -77, dtype=np.int32)
        start = np.full((B, K), -77, dtype=np.int32)
        length = np.full((B, K), -77, dtype=np.int32)
        assert lib.viai_gap_detect_host(wav.ctypes.data, None, n, B, n, 0.0, 0.0, 4, 0, K, count.ctypes.data, start.ctypes.data,
                                        length.ctypes.data) == 0
        want = G.rule(wav, n, min_len=4, max_gaps=K)
        assert np.array_equal(count, want[0]) and np.array_equal(start, want[1]) and np.array_equal(length, want[2])


def test_python_entry_points_check_their_arguments():
    from viai_amd import gap_detect
    from viai_amd._lib import ViaiLibraryError
    with pytest.raises(ViaiLibraryError):
        gap_detect.find_gaps(torch.zeros(2, 100))                         # a CPU tensor: no fallback
    for bad in (dict(min_len=0), dict(merge_within=-1), dict(max_gaps=0), dict(threshold=-1.0), dict(threshold=float("nan")), dict(clip=-0.5),
                dict(clip=float("nan")), dict(min_len=1.5)):
        with pytest.raises(ValueError):
            gap_detect.find_gaps_host(np.zeros((1, 8), dtype=np.float32), **bad)
        with pytest.raises(ValueError):
            gap_detect.find_gaps(torch.zeros(1, 8), **bad)
    with pytest.raises(ValueError):
        gap_detect.find_gaps_host(np.zeros(8, dtype=np.float32))
    with pytest.raises(ValueError):
        gap_detect.find_gaps_host(np.zeros((2, 8), dtype=np.float32), lengths=[1, 2, 3])
    got = gap_detect.find_gaps_host(np.zeros((2, 8)), min_len=1, max_gaps=2)                              # float64 in: converted
    assert isinstance(got, gap_detect.Gaps) and got._fields == ("count", "start", "length") and list(got.count) == [1, 1]


# ----------------------------------------------------------------------------- 3. the workspace size
def test_workspace_bytes_are_positive_and_monotone(lib):
    ws = lib.viai_gap_detect_ws_bytes
    assert ws(1, 1, 1) > 0
    for B, n, K in ((1, 1, 1), (3, G.T, 16), (8, 1 << 20, 16), (8, 1 << 24, 64)):
        base = ws(B, n, K)
        assert base >= (n + 7) // 8 * B                                  # at least the 1-bit-per-sample mask
        assert ws(B + 1, n, K) > base and ws(B, n + G.T, K) > base and ws(B, n + 1, K) >= base and ws(B, n, K + 1) >= base
    sizes = [ws(2, n, 4) for n in (1, 100, G.T, G.T + 1, 10 * G.T, 1 << 22, (1 << 31) - 1)]
    assert sizes == sorted(sizes) and sizes[0] > 0
    assert [ws(B, 5 * G.T, 4) for B in (1, 2, 4, 8)] == [ws(1, 5 * G.T, 4) * B for B in (1, 2, 4, 8)]
    for B, n, K in ((0, 100, 4), (-1, 100, 4), (1, 0, 4), (1, -5, 4), (1, 100, 0), (1, 100, -1), (1, 1 << 31, 4), (1, 1 << 40, 4),
                    (1 << 30, 1 << 30, 4)):
        assert ws(B, n, K) == 0, (B, n, K)


# ----------------------------------------------------------------------------- 4. refusals, before any launch
def test_every_refusal_is_invalid_value_without_a_device(lib):
    """the pointers are never dereferenced by a refused call: small fake addresses, aligned as the call wants them"""
    wav, cnt, st, ln, ws = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000
    nan = float("nan")

    def call(wav=wav, lengths=None, stride=100, B=2, n=100, threshold=0.0, clip=0.0, min_len=4, merge_within=0, K=4, count=cnt, start=st,
             length=ln, ws=ws):
        return lib.viai_gap_detect(wav, lengths, stride, B, n, threshold, clip, min_len, merge_within, K, count, start, length, ws, None)

    def call_host(wav=wav, lengths=None, stride=100, B=2, n=100, threshold=0.0, clip=0.0, min_len=4, merge_within=0, K=4, count=cnt, start=st,
                  length=ln, ws=None):
        return lib.viai_gap_detect_host(wav, lengths, stride, B, n, threshold, clip, min_len, merge_within, K, count, start, length)
    bad = [dict(wav=None), dict(count=None), dict(start=None), dict(length=None), dict(ws=None), dict(B=0), dict(B=-1), dict(n=0), dict(n=-4),
           dict(K=0), dict(K=-2), dict(n=1 << 31, stride=1 << 31), dict(n=1 << 33, stride=1 << 33), dict(stride=99), dict(stride=0),
           dict(min_len=0), dict(min_len=-1), dict(merge_within=-1), dict(threshold=-1e-30), dict(threshold=nan), dict(threshold=-float("inf")),
           dict(clip=-0.5), dict(clip=nan)]
    for kw in bad:
        assert call(**kw) == INVALID, kw
        if "ws" not in kw:
            assert call_host(**kw) == INVALID, kw
