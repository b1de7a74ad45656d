"""No GPU: the host mirror of the click detector (`viai_click_detect_host`, plain loops over csrc/viai_click_rule.h) against two numpy
restatements of include/viai_hip.h's rule, its structure, and what it detects.  Needs the built library.

3. THE MARGIN.  The restatement with ordinary sums (np.dot, np.convolve, np.sum) differs from the rule's summation order in the last bits of
q / threshold.  The margin is MEASURED by the test itself (`click_detect_common.measured_margin`): the largest relative difference of q / threshold between the two
restatements over the judged samples of the whole table, times 4: 7.5e-9 over 226 088 samples on the table as committed
(tools/click_detect_rate.py writes it to profiles/click_detect_rate.json).  Flags must agree on every sample whose q / threshold is farther
than the margin from 1, and at most one sample per 4096 may lie that close: a condition on the table, to be met by choosing another seed.

4. DETECTION.  Seeds 0 to 5 of the base signal, 12 clicks of +-20 s each: every click inside a listed run, every run within
[c - guard, c + order + guard] of a click c, the clean signal without a run.  SNR over the clicked samples against the clean signal, before ->
after `declick_host`, is printed per seed (and recorded in profiles/click_detect_rate.json); the test asserts only that the gain is positive."""
import numpy as np
import pytest

import click_detect_common as K


def built_lib():
    from viai_amd import _lib
    try:
        return _lib.load()
    except _lib.ViaiLibraryError as e:                                     # pragma: no cover
        pytest.fail("the library is not built: %s" % e)


def host(c, **over):
    from viai_amd.click_detect import find_clicks_host
    built_lib()
    return find_clicks_host(K.clip(c), **dict(K.call_kwargs(c), **over))


def runs(g, b=0):
    n = min(int(g.count[b]), g.start.shape[1])
    return [(int(g.start[b, i]), int(g.length[b, i])) for i in range(n)]


# ----------------------------------------------------------------------------- 1. the host mirror is the rule, as exact integers
@pytest.mark.parametrize("name", K.case_names())
def test_host_mirror_equals_the_restatement_exactly(name):
    c = K.case_by_name(name)
    got, want = host(c), K.rule_exact(c)
    assert got.count.dtype == np.int32 and got.start.shape == want.start.shape
    assert np.array_equal(got.count, want.count), (got.count, want.count)
    assert np.array_equal(got.start, want.start) and np.array_equal(got.length, want.length)


def test_host_mirror_equals_the_restatement_on_a_long_row():
    """257 tiles (click_detect_common.long_case): the runs that the GPU test compares the device with are the restatement's, and they are where
    the clicks were planted -- across both thread edges, in the last full tile, nothing in row 0's one-sample last tile"""
    c = K.long_case()
    got, want = host(c), K.rule_exact(c)
    assert np.array_equal(got.count, want.count) and np.array_equal(got.start, want.start) and np.array_equal(got.length, want.length)
    E, g = 2 * K.TILE, K.DEFAULTS["guard"]
    assert 0 < int(got.count.max()) <= K.DEFAULTS["max_gaps"]
    for b, ln in enumerate(K.LONG_LENGTHS):
        rs = runs(got, b)
        for edge in (E, 64 * E):
            assert any(st <= edge - 2 * g and edge + 2 * g < st + n for st, n in rs), (b, edge)        # one run over the edge, guards included
        assert all(st + n <= ln for st, n in rs)
    covers = lambda rs, at: any(st <= at < st + n for st, n in rs)
    assert covers(runs(got, 0), 255 * K.TILE + 100) and covers(runs(got, 0), 255 * K.TILE + 2000) and not covers(runs(got, 0), K.LONG_N - 1)
    assert not covers(runs(got, 1), 255 * K.TILE + 100)                    # behind row 1's length


def test_the_table_finds_something():
    """the comparison above is not one of empty lists"""
    assert runs(host(K.case_by_name("base"))) and int(host(K.case_by_name("overflow")).count[0]) == 12


# ----------------------------------------------------------------------------- 2. structure
def test_the_head_of_a_row_is_never_judged_unless_non_finite():
    from viai_amd.click_detect import find_clicks_host
    clean, s = K.base_signal(0)
    x = clean.copy()
    x[:32] += np.float32(50 * s) * np.where(np.arange(32) % 2 == 0, 1, -1).astype(np.float32)       # wild, but in front of sample p = 32
    g = find_clicks_host(x[None, :], guard=0, merge_within=0)
    assert all(st >= 32 for st, _ in runs(g))
    x[7] = np.float32("nan")
    g = find_clicks_host(x[None, :], guard=0, merge_within=0)
    assert runs(g)[0] == (7, 1)


def test_a_nan_is_always_flagged():
    from viai_amd.click_detect import find_clicks_host
    clean, _ = K.base_signal(1)
    for at in (0, 31, 32, 4095, 4096, K.N_BASE - 1):
        x = clean.copy()
        x[at] = np.float32("nan")
        assert runs(find_clicks_host(x[None, :], guard=0))[0][0] == at, at      # it reads as 0.0, so samples behind it may be outliers too
        x = np.zeros(K.N_BASE, dtype=np.float32)                            # in a row of zeros every residual is 0: the NaN alone
        x[at] = np.float32("nan")
        assert runs(find_clicks_host(x[None, :], guard=0)) == [(at, 1)], at
    x = np.full((1, 4097), np.float32(0.1))
    x[0, 4096] = np.float32("inf")                                          # a one-sample last tile: p < 1, still flagged
    assert runs(find_clicks_host(x, guard=0)) == [(4096, 1)]


def test_constant_and_zero_rows_hold_nothing():
    g = host(K.case_by_name("constant and zero rows"))
    assert g.count.tolist() == [0, 0] and not g.start.any() and not g.length.any()


def test_guard_crosses_words_and_tiles_and_stops_at_len():
    from viai_amd.click_detect import find_clicks_host
    for at, guard, ln, want in ((64, 3, K.N_BASE, (61, 7)), (4096, 5, K.N_BASE, (4091, 11)), (4095, 64, K.N_BASE, (4031, 129)),
                                (5000, 64, 5003, (4936, 67)), (33, 64, K.N_BASE, (0, 98))):
        x = np.zeros(K.N_BASE, dtype=np.float32)                            # every residual is 0: the one flag is the NaN's
        x[at] = np.float32("nan")
        assert runs(find_clicks_host(x[None, :], lengths=[ln], guard=guard)) == [want], (at, guard)


def test_a_one_sample_last_tile_flags_nothing():
    from viai_amd.click_detect import find_clicks_host
    clean, s = K.base_signal(3, n=4097)
    x = clean.copy()
    x[4096] += np.float32(1000 * s)                                         # finite and wild, but the tile has p = 0
    assert int(find_clicks_host(x[None, :]).count[0]) == 0
    x[4095] += np.float32(1000 * s)                                         # the sample before it is the first tile's
    assert runs(find_clicks_host(x[None, :], guard=0)) == [(4095, 1)]


def test_passes_matter_next_to_a_huge_click():
    from viai_amd.click_detect import find_clicks_host
    clean, s = K.base_signal(4)
    x = clean.copy()
    x[1000] += np.float32(200 * s)
    x[3000] += np.float32(12 * s)
    plain = runs(find_clicks_host(x[None, :], passes=0))
    robust = runs(find_clicks_host(x[None, :], passes=2))
    covers = lambda rs, at: any(st <= at < st + ln for st, ln in rs)
    assert covers(plain, 1000) and covers(robust, 1000)
    assert not covers(plain, 3000) and covers(robust, 3000)                # the plain mean is dragged up by the huge click


def test_overflow_reports_the_true_count():
    c = K.case_by_name("overflow")
    few, many = host(c), host(c, max_gaps=64)
    assert int(few.count[0]) == 12 == int(many.count[0]) and few.start.shape == (1, 4)
    assert np.array_equal(few.start[0], many.start[0, :4]) and np.array_equal(few.length[0], many.length[0, :4])


def test_argument_errors():
    from viai_amd import _lib
    from viai_amd.click_detect import declick, find_clicks, find_clicks_host
    import torch
    x = np.zeros((2, 100), dtype=np.float32)
    for kw in (dict(order=0), dict(order=129), dict(order=1.5), dict(k=0.0), dict(k=-1.0), dict(k=float("inf")), dict(k=float("nan")),
               dict(passes=-1), dict(passes=5), dict(guard=-1), dict(guard=65), dict(floor=-0.1), dict(floor=float("nan")), dict(min_len=0),
               dict(merge_within=-1), dict(max_gaps=0), dict(lengths=[1, 2, 3])):
        with pytest.raises(ValueError):
            find_clicks_host(x, **kw)
        with pytest.raises(ValueError):
            find_clicks(torch.zeros(2, 100), **kw)
    with pytest.raises(ValueError):
        find_clicks_host(np.zeros(100, dtype=np.float32))
    with pytest.raises(_lib.ViaiLibraryError, match="GPU only"):
        find_clicks(torch.zeros(2, 100))
    with pytest.raises(_lib.ViaiLibraryError, match="GPU only"):
        declick(torch.zeros(2, 100))
    lib = built_lib()
    assert lib.viai_click_detect_ws_bytes(0, 100, 4) == 0 and lib.viai_click_detect_ws_bytes(1, 2 ** 31, 4) == 0
    assert lib.viai_click_detect_ws_bytes(3, 4097, 4) == 3 * 2 * (2 * 512 + 52)
    assert lib.viai_click_detect_host(None, None, 100, 1, 100, 32, 5.0, 2, 2, 0.0, 1, 8, 4, None, None, None) != 0


def test_the_package_exports_the_calls():
    import viai_amd
    from viai_amd import click_detect
    for name in ("find_clicks", "find_clicks_host", "declick", "declick_host", "declick_file"):
        assert getattr(viai_amd, name) is getattr(click_detect, name)


# ----------------------------------------------------------------------------- 3. against ordinary sums
def test_flags_agree_with_ordinary_sums_outside_the_margin():
    margin, seen = K.measured_margin()
    print("measured margin %.3e over %d judged samples" % (margin, seen))
    assert seen > 100000 and margin < 1e-6                                 # 7.5e-9 when this was written; 1e-6 is the table's own clearance
    for c in K.all_cases():
        for b, ((_, f1, judged, r1), (_, f2, _, r2)) in enumerate(zip(K.masks(c, exact=True), K.masks(c, exact=False))):
            close = judged & (np.abs(r1 - 1.0) <= margin)
            assert int(close.sum()) <= max(1, judged.size // 4096), (c["name"], b)       # the condition on the table
            assert np.array_equal(f1[~close], f2[~close]), (c["name"], b)


# ----------------------------------------------------------------------------- 4. detection
@pytest.mark.parametrize("seed", range(6))
def test_detection_on_the_base_signal(seed):
    from viai_amd.click_detect import declick_host, find_clicks_host
    built_lib()
    clean, hurt, pos, s = K.clicked(seed)
    order, guard = 32, 2
    g = find_clicks_host(hurt[None, :])
    rs = runs(g)
    assert int(g.count[0]) == len(rs)
    for c in pos:
        assert any(st <= c < st + ln for st, ln in rs), ("missed", c)
    for st, ln in rs:
        assert any(c - guard <= st and st + ln - 1 <= c + order + guard for c in pos), ("stray", st, ln)
    assert int(find_clicks_host(clean[None, :]).count[0]) == 0
    out, g2, filled = declick_host(hurt[None, :])
    assert np.array_equal(g2.start, g.start) and (filled[0, :len(rs)] > 0).all()
    before, after = K.snr_db(clean, hurt, pos), K.snr_db(clean, out[0], pos)
    print("seed %d: %d runs, SNR over the clicked samples %.2f dB -> %.2f dB (gain %.2f dB)" % (seed, len(rs), before, after, after - before))
    assert after - before > 0.0
    inside = np.zeros(hurt.size, dtype=bool)
    for st, ln in rs:
        inside[st:st + ln] = True
    assert np.array_equal(out[0][~inside].view(np.int32), hurt[~inside].view(np.int32))
