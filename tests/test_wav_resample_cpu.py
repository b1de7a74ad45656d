"""The polyphase resampler (`viai_amd.wav_resample`, csrc/wav_resample.hip), the parts that need no GPU: the C symbols, the plan, the tap table
against the fp64 restatement, what the filter does to tones, the widening of a gap against brute force, the refusals in front of the launch and
the argument checks in front of the device."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import wav_resample_common as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PL = C.POINTER(C.c_long)
PI = C.POINTER(C.c_int)
NEW = {"viai_wav_resample_geom": (C.c_int, 7), "viai_wav_resample_taps": (C.c_int, 7), "viai_wav_resample_out_len": (C.c_long, 3),
       "viai_gap_at_rate": (C.c_int, 8), "viai_wav_resample": (C.c_int, 16), "viai_wav_resample_form": (C.c_int, 7)}
INVAL = 1                                                                # hipErrorInvalidValue
_TABLES = {}


@pytest.fixture(scope="module")
def lib():
    from viai_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def geom(lib, sr_in, sr_out, zeros=24):
    v = [C.c_int() for _ in range(4)]
    err = lib.viai_wav_resample_geom(sr_in, sr_out, zeros, *[C.byref(x) for x in v])
    return err, tuple(x.value for x in v)


def lib_table(lib, sr_in, sr_out):
    """the library's table as ((L, T) float32 in period order, first), computed once per ratio"""
    if (sr_in, sr_out) not in _TABLES:
        L, M, H, T = R.plan(sr_in, sr_out)
        taps = np.zeros((T, L), dtype=np.float32)
        first = np.zeros(L, dtype=np.int32)
        assert lib.viai_wav_resample_taps(sr_in, sr_out, 24, 0.945, 8.6, taps.ctypes.data, first.ctypes.data) == 0
        _TABLES[(sr_in, sr_out)] = (np.ascontiguousarray(taps.T), first)
    return _TABLES[(sr_in, sr_out)]


def test_new_symbols_are_declared_typed_and_exported(lib):
    from viai_amd import _lib
    with open(os.path.join(ROOT, "include", "viai_hip.h")) as f:
        header = f.read()
    for name, (res, nargs) in NEW.items():
        got_res, args = _lib.SIGNATURES[name]
        assert got_res is res and len(args) == nargs, name
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args)
        assert ("%s %s(" % ("long" if res is C.c_long else "int", name)) in header
    assert lib.viai_abi_version() == 20 == _lib.ABI_VERSION
    assert "wav_resample.hip" in open(os.path.join(ROOT, "vision-infused-audio-inpainter-viai_amd", "csrc", "Makefile")).read()
    assert "#define VIAI_WAV_RESAMPLE_MAX_TABLE 4194304" in header


def test_plan_of_the_six_ratios(lib):
    for (sr_in, sr_out), want in R.RATIOS.items():
        assert geom(lib, sr_in, sr_out) == (0, want), (sr_in, sr_out)
        assert R.plan(sr_in, sr_out) == want
    assert geom(lib, 8000, 16000, 7) == (0, (2, 1, 7, 15))
    assert geom(lib, 16000, 8000, 7) == (0, (1, 2, 14, 29))
    for bad in ((0, 16000, 24), (16000, 0, 24), (-1, 16000, 24), (16000, 44100, 0)):
        assert geom(lib, *bad)[0] == INVAL, bad
    assert geom(lib, 1000003, 1000033)[0] == INVAL                       # coprime rates: a table of 49 x 1000033 taps is over the cap
    assert geom(lib, 44100, 44101)[0] == 0                               # 49 x 44101 is not
    none = C.cast(None, PI)
    assert lib.viai_wav_resample_geom(44100, 16000, 24, none, none, none, none) == INVAL


def test_output_length(lib):
    f = lib.viai_wav_resample_out_len
    for L, M, _, _ in R.RATIOS.values():
        top = (2 ** 31 - 1) * M // L                                     # the largest n whose output length fits an int32
        for n in (1, M, M + 1, top):
            assert f(n, L, M) == -(-n * L // M), (n, L, M)
        assert f(top, L, M) <= 2 ** 31 - 1 < f(top + 1, L, M)
        assert f(0, L, M) == 0 and f(-1, L, M) == 0
    assert f(5, 0, 1) == 0 and f(5, 1, 0) == 0


def form(lib, L, M, H):
    v = [C.c_int(-7) for _ in range(4)]
    err = lib.viai_wav_resample_form(L, M, H, *[C.byref(x) for x in v])
    return err, tuple(x.value for x in v)


def kind(L, f):
    """which of the eight answers of the rule a form is"""
    return (f[0], f[1] if f[0] == 1 else 0, L <= R.PERIOD_MAX_L if f[0] == 0 else None)


KINDS = {(4, 0, None)} | {(1, lt, None) for lt in (1024, 512, 256, 128, 64)} | {(0, 0, True), (0, 0, False)}


def test_every_launch_form_has_a_named_plan_that_takes_it(lib):
    """the library's answer (`viai_wav_resample_form`), the restatement `R.pick` and the table of wav_resample_common.py agree plan by plan, and
    the named plans between them take every form the rule can return"""
    from viai_amd import wav_resample as WR
    named = dict(R.PERIOD_FORMS)
    named.update({rates: f for rates, (_, f) in R.FORMS.items()})
    named.update({rates: (0, 0, 0, 0) for rates in R.REFUSED})
    plans = dict(R.RATIOS)
    plans.update({rates: p for rates, (p, _) in R.FORMS.items()})
    plans.update(R.REFUSED)
    seen = set()
    for rates, want in named.items():
        L, M, H, T = plans[rates]
        assert geom(lib, *rates) == (0, (L, M, H, T)) and R.plan(*rates) == (L, M, H, T), rates
        assert L * T <= R.MAX_TABLE
        assert form(lib, L, M, H) == (0, want), rates
        assert R.pick(L, M, H) == want, rates
        assert WR.Resampler(*rates).launch_form() == want                # the table is not built for this
        pp, lt, g, words = want
        if pp:
            assert words == R.span(lt * g * pp, L, M, H) <= R.MAX_SPAN and (g == 1 if pp == 1 else lt == L)
        seen.add(kind(L, want))
    assert seen == KINDS
    # each named plan is named for something: the consecutive form above the period limit and below it, the budget's edge, one item per block
    assert R.FORMS[(11025, 16000)][0][0] > R.PERIOD_MAX_L >= R.FORMS[(4001, 400)][0][0] and R.FORMS[(4001, 400)][1][0] == 1
    assert R.span(4 * 400, 400, 4001, 241) > R.MAX_SPAN                  # why 4001 -> 400 falls through: g = 1 of the period form does not fit
    assert R.MAX_SPAN - 32 < R.FORMS[(28135, 521)][1][3] <= R.MAX_SPAN
    assert R.FORMS[(300, 1)][1][:3] == (4, 1, 1) and 4 * R.FORMS[(300, 1)][1][3] > 60000
    assert R.REFUSED[(330, 1)][0] <= R.PERIOD_MAX_L < R.REFUSED[(77109, 521)][0]
    # refused like the plan's other queries
    none = C.cast(None, PI)
    assert lib.viai_wav_resample_form(160, 441, 67, none, none, none, none) == INVAL
    for bad in ((0, 441, 67), (160, 0, 67), (160, 441, -1), (-3, 441, 67)):
        assert form(lib, *bad)[0] == INVAL, bad
    assert form(lib, 2, 1, 0) == (0, R.pick(2, 1, 0))                    # H = 0 is a plan the launch takes too


def test_the_restated_rule_is_the_librarys_over_random_plans(lib):
    """a few hundred (sr_in, sr_out, zeros), drawn so that every answer of the rule turns up, refused plans included"""
    rng = np.random.default_rng(2024)
    seen, checked, no_plan = set(), 0, 0
    draws = []
    for _ in range(120):                                                  # everyday rates both ways: short periods, small M / L
        a, b = rng.choice([8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 96000], 2, replace=False)
        draws.append((int(a), int(b), int(rng.integers(1, 65))))
    for _ in range(160):                                                  # coprime-ish pairs: long periods
        draws.append((int(rng.integers(1, 40000)), int(rng.integers(1, 40000)), int(rng.integers(1, 33))))
    for _ in range(200):                                                  # steep decimation: M / L from 2 to 400, where the span decides
        L = int(rng.choice([1, 2, 3, 7, 100, 400, 512, 513, 521, 1000]))
        draws.append((L * int(rng.integers(2, 400)) + int(rng.integers(0, L + 1)), L, int(rng.integers(1, 49))))
    for sr_in, sr_out, zeros in draws:
        err, got = geom(lib, sr_in, sr_out, zeros)
        L, M, H, T = R.plan(sr_in, sr_out, zeros)
        if err != 0:
            assert err == INVAL and L * T > R.MAX_TABLE, (sr_in, sr_out, zeros)
            no_plan += 1
            continue
        assert got == (L, M, H, T) and L * T <= R.MAX_TABLE
        want = R.pick(L, M, H)
        assert form(lib, L, M, H) == (0, want), (sr_in, sr_out, zeros)
        # the launch itself refuses exactly the plans without a form, before anything is launched (the pointers are never followed)
        refused = lib.viai_wav_resample(16, None, 16, 16, 16, None, None, 1, 100, 100, 1, L, M, H, T, None) if want[0] == 0 else INVAL
        assert refused == INVAL
        seen.add(kind(L, want))
        checked += 1
    assert seen == KINDS and checked >= 300 and no_plan > 0
    print("random plans: %d checked, %d over the table cap" % (checked, no_plan))


def new_plans():
    return list(R.FORMS) + [(330, 1), (77109, 521)]


@pytest.mark.parametrize("rates", new_plans())
def test_taps_of_the_new_plans_are_the_restatement_rounded_once(lib, rates):
    """what test_taps_are_the_restatement_rounded_once asserts of the six, of every plan of FORMS and of two refused ones (their tables exist)"""
    L, M, H, T = R.plan(*rates)
    got, first = lib_table(lib, *rates)
    want, want_first = R.table(*rates)
    assert got.shape == (L, T) == want.shape
    assert np.array_equal(first, want_first)
    rounded = want.astype(np.float32)
    ulp = np.spacing(np.abs(rounded))
    assert np.all(np.abs(got.astype(np.float64) - rounded.astype(np.float64)) <= ulp.astype(np.float64))
    assert np.array_equal(got == 0, rounded == 0)
    sums = got.astype(np.float64).sum(1)
    print("%s: largest |row sum - 1| %.3g" % (rates, float(np.abs(sums - 1).max())))
    assert np.abs(sums - 1).max() < 3e-5
    assert np.all(got[:, 0] == 0)


@pytest.mark.parametrize("rates", list(R.FORMS))
def test_the_fp32_chain_stays_inside_the_bound_for_the_new_plans(lib, rates):
    """test_the_fp32_chain_stays_inside_the_dot_product_bound at the new plans' T (up to 14 401 terms) and the GPU test's sizes"""
    L, M, H, T = R.plan(*rates)
    h = lib_table(lib, *rates)[0].astype(np.float64)
    n, m = R.value_size(rates)
    x = np.random.default_rng(L + M).uniform(-1, 1, n).astype(np.float32)
    want, mags = R.resample(x, L, M, H, h)
    got, _ = R.resample(x, L, M, H, h, dtype=np.float32)
    bound = (T + 4) * 2.0 ** -24 * mags
    assert want.shape == (m,) and np.all(np.abs(got - want) <= bound)
    print("%s: n = %d, m = %d, fp32 chain: largest error over the bound %.3f" % (rates, n, m, float((np.abs(got - want) / bound).max())))


@pytest.mark.parametrize("rates", [(11025, 16000), (4001, 400), (8337, 521)])
def test_gap_at_rate_against_brute_force_for_consecutive_form_plans(lib, rates):
    """test_gap_at_rate_against_brute_force for plans that take the consecutive form: up, and down with filters of 483 and 771 taps"""
    L, M, H, T = R.plan(*rates)
    h = lib_table(lib, *rates)[0].astype(np.float64)
    n = 2000
    m = R.out_len(n, L, M)
    rng = np.random.default_rng(5)
    x = rng.uniform(-1, 1, n)
    y = R.resample(x, L, M, H, h)[0]
    k0, k1 = C.c_long(-7), C.c_long(-7)
    for g0, g1 in ((0, 100), (0, 1), (900, 1100), (1000, 1001), (1900, 2000), (1999, 2000), (700, 700), (800, 790)):
        assert lib.viai_gap_at_rate(g0, g1, L, M, H, m, C.byref(k0), C.byref(k1)) == 0
        a, b = k0.value, k1.value
        assert (a, b) == R.gap_at_rate(g0, g1, L, M, H, m), (g0, g1)
        if g1 <= g0:
            assert (a, b) == (0, 0)
            continue
        other = x.copy()
        other[g0:g1] = rng.uniform(-1, 1, g1 - g0) + 2.0
        d = R.resample(other, L, M, H, h)[0] - y
        assert np.all(d[:a] == 0) and np.all(d[b:] == 0), (g0, g1)
        assert 0 <= a < b <= m
        lo, hi = R.support(a, L, M, H)
        assert a == 0 or (hi >= g0 and lo < g1)
        assert a == 0 or R.support(a - 1, L, M, H)[1] < g0
        lo, hi = R.support(b - 1, L, M, H)
        assert b == m or (hi >= g0 and lo < g1)
        assert b == m or R.support(b, L, M, H)[0] >= g1


def test_taps_are_the_restatement_rounded_once(lib):
    worst = 0.0
    for (sr_in, sr_out), (L, M, H, T) in R.RATIOS.items():
        got, first = lib_table(lib, sr_in, sr_out)
        want, want_first = R.table(sr_in, sr_out)
        assert got.shape == (L, T) == want.shape
        assert np.array_equal(first, want_first)
        rounded = want.astype(np.float32)
        ulp = np.spacing(np.abs(rounded))
        assert np.all(np.abs(got.astype(np.float64) - rounded.astype(np.float64)) <= ulp.astype(np.float64)), (sr_in, sr_out)
        assert np.array_equal(got == 0, rounded == 0)                    # the window ends where the formula says
        sums = got.astype(np.float64).sum(1)
        worst = max(worst, float(np.abs(sums - 1).max()))
        assert np.abs(sums - 1).max() < 3e-5, (sr_in, sr_out)
        assert np.all(got[:, 0] == 0)                                    # t = r / L + H >= W at j = 0: the first tap is outside the window
    print("largest |row sum - 1| over the six ratios: %.3g" % worst)
    # refused like the plan, and for a roll-off or a beta outside their ranges
    buf, ints = np.zeros(64, dtype=np.float32), np.zeros(8, dtype=np.int32)
    taps = lib.viai_wav_resample_taps
    assert taps(0, 16000, 24, 0.945, 8.6, buf.ctypes.data, ints.ctypes.data) == INVAL
    assert taps(48000, 16000, 24, 0.0, 8.6, buf.ctypes.data, ints.ctypes.data) == INVAL
    assert taps(48000, 16000, 24, 1.5, 8.6, buf.ctypes.data, ints.ctypes.data) == INVAL
    assert taps(48000, 16000, 24, 0.945, -1.0, buf.ctypes.data, ints.ctypes.data) == INVAL
    assert taps(48000, 16000, 24, 0.945, 8.6, None, ints.ctypes.data) == INVAL
    assert taps(48000, 16000, 24, 0.945, 8.6, buf.ctypes.data, None) == INVAL


def test_filter_quality_with_the_library_taps(lib):
    """44.1 kHz -> 16 kHz, 8192-sample tones, 200 outputs trimmed at each end: pass band and stop band; 16 -> 44.1 -> 16 kHz round trip"""
    L, M, H, T = R.RATIOS[(44100, 16000)]
    h = lib_table(lib, 44100, 16000)[0].astype(np.float64)
    n = 8192
    i = np.arange(n)
    m = R.out_len(n, L, M)
    k = np.arange(m)[200:-200]
    figures = {}
    tone = np.sin(2 * np.pi * 6500.0 * i / 44100.0 + 0.3)
    y = R.resample(tone, L, M, H, h)[0][200:-200]
    ideal = np.sin(2 * np.pi * 6500.0 * k / 16000.0 + 0.3)
    figures["6.5 kHz"] = R.db(y - ideal, ideal)
    assert figures["6.5 kHz"] < -90
    for f in (9000.0, 12000.0):
        tone = np.sin(2 * np.pi * f * i / 44100.0 + 0.3)
        y = R.resample(tone, L, M, H, h)[0][200:-200]
        figures["%g kHz" % (f / 1000)] = R.db(y, tone)
        assert figures["%g kHz" % (f / 1000)] < -90, f
    Lu, Mu, Hu, Tu = R.RATIOS[(16000, 44100)]
    hu = lib_table(lib, 16000, 44100)[0].astype(np.float64)
    x = sum(a * np.sin(2 * np.pi * f * i / 16000.0 + p) for f, a, p in ((310.0, 0.3, 0.1), (1234.5, 0.25, 1.0), (3000.0, 0.2, 2.0),
                                                                          (5100.0, 0.15, 0.5), (6150.0, 0.1, 2.5)))
    up = R.resample(x, Lu, Mu, Hu, hu)[0]
    back = R.resample(up, L, M, H, h, m=n)[0]
    figures["round trip"] = R.db((back - x)[200:-200], x[200:-200])
    assert figures["round trip"] < -90
    print("filter quality in dB: " + ", ".join("%s %.1f" % kv for kv in figures.items()))


def test_the_fp32_chain_stays_inside_the_dot_product_bound(lib):
    """what the GPU test asserts of the kernel, asserted here of the same chain on the CPU: fp32 multiply-adds in tap order on the library's taps
    stay within (T + 4) 2^-24 sum |x| |h| of the fp64 sum over the same taps, at the GPU test's row length"""
    worst = 0.0
    for rates, (L, M, H, T) in R.RATIOS.items():
        h = lib_table(lib, *rates)[0].astype(np.float64)
        n = 5 * max(L, M) + 7
        x = np.random.default_rng(L + M).uniform(-1, 1, n).astype(np.float32)
        want, mags = R.resample(x, L, M, H, h)
        got, _ = R.resample(x, L, M, H, h, dtype=np.float32)
        bound = (T + 4) * 2.0 ** -24 * mags
        assert np.all(np.abs(got - want) <= bound), rates
        worst = max(worst, float((np.abs(got - want) / bound).max()))
    print("fp32 chain: largest error over the bound %.3f" % worst)


@pytest.mark.parametrize("rates", [(44100, 16000), (16000, 44100)])
def test_gap_at_rate_against_brute_force(lib, rates):
    L, M, H, T = R.RATIOS[rates]
    h = lib_table(lib, *rates)[0].astype(np.float64)
    n = 2000
    m = R.out_len(n, L, M)
    rng = np.random.default_rng(5)
    x = rng.uniform(-1, 1, n)
    y = R.resample(x, L, M, H, h)[0]
    k0, k1 = C.c_long(-7), C.c_long(-7)
    for g0, g1 in ((0, 100), (0, 1), (900, 1100), (1000, 1001), (1900, 2000), (1999, 2000), (700, 700), (800, 790)):
        assert lib.viai_gap_at_rate(g0, g1, L, M, H, m, C.byref(k0), C.byref(k1)) == 0
        a, b = k0.value, k1.value
        assert (a, b) == R.gap_at_rate(g0, g1, L, M, H, m), (g0, g1)
        if g1 <= g0:
            assert (a, b) == (0, 0)
            continue
        other = x.copy()
        other[g0:g1] = rng.uniform(-1, 1, g1 - g0) + 2.0
        d = R.resample(other, L, M, H, h)[0] - y
        assert np.all(d[:a] == 0) and np.all(d[b:] == 0), (g0, g1)      # exactly: no term of those sums changed
        assert 0 <= a < b <= m
        lo, hi = R.support(a, L, M, H)
        assert a == 0 or (hi >= g0 and lo < g1)                          # the first one reads a sample of the gap, or the clip starts there
        assert a == 0 or R.support(a - 1, L, M, H)[1] < g0               # and the one before it does not
        lo, hi = R.support(b - 1, L, M, H)
        assert b == m or (hi >= g0 and lo < g1)
        assert b == m or R.support(b, L, M, H)[0] >= g1
    assert lib.viai_gap_at_rate(0, 10, L, M, H, 5, C.byref(k0), C.byref(k1)) == 0 and k1.value <= 5      # clipped to m
    assert lib.viai_gap_at_rate(10 ** 6, 10 ** 6 + 10, L, M, H, m, C.byref(k0), C.byref(k1)) == 0 and (k0.value, k1.value) == (0, 0)
    assert lib.viai_gap_at_rate(0, 10, 0, M, H, m, C.byref(k0), C.byref(k1)) == INVAL
    assert lib.viai_gap_at_rate(0, 10, L, M, H, m, C.cast(None, PL), C.byref(k1)) == INVAL


def test_refused_launches_return_invalid_value_before_any_launch(lib):
    one = 16                                                             # a stand-in for a device pointer that is never followed
    run = lib.viai_wav_resample
    L, M, H, T = 160, 441, 67, 135

    def call(x=one, lengths=one, taps=one, first=one, y=one, o0=one, o1=one, B=2, xs=1000, ys=400, m=363, L=L, M=M, H=H, T=T):
        return run(x, lengths, taps, first, y, o0, o1, B, xs, ys, m, L, M, H, T, None)
    for name in ("x", "taps", "first", "y"):                             # the required pointers
        assert call(**{name: None}) == INVAL, name
    for name in ("B", "m", "L", "M", "T"):
        assert call(**{name: 0}) == INVAL, name
        assert call(**{name: -3}) == INVAL, name
    assert call(T=T + 2) == INVAL and call(H=H + 1) == INVAL             # T != 2 H + 1
    assert call(H=-1, T=-1) == INVAL
    assert call(ys=362) == INVAL                                         # y_stride shorter than what is written
    assert call(xs=0) == INVAL
    assert call(x=18) == INVAL and call(y=18) == INVAL                   # no float pointers
    assert call(L=44101, M=44100, H=1000, T=2001) == INVAL               # a table over the cap
    assert call(L=1, M=40000, H=24 * 40000, T=48 * 40000 + 1) == INVAL   # a halo no tile can stage


def test_python_argument_errors_are_raised_before_the_device(lib):
    from viai_amd import wav_resample as WR
    with pytest.raises(ValueError, match="no resampling"):
        WR.Resampler(16000, 16000)
    with pytest.raises(ValueError, match="no plan"):
        WR.Resampler(0, 16000)
    with pytest.raises(ValueError, match="no plan"):
        WR.Resampler(44100, 16000, zeros=0)
    with pytest.raises(ValueError, match="integers"):
        WR.Resampler(44100.5, 16000)
    with pytest.raises(ValueError, match="rolloff"):
        WR.Resampler(44100, 16000, rolloff=1.2)
    rs = WR.Resampler(44100, 16000)
    assert (rs.L, rs.M, rs.H, rs.T) == R.RATIOS[(44100, 16000)]
    assert rs.out_len(20400) == 7402 and WR.Resampler(48000, 16000).out_len(22272) == 7424
    x = torch.zeros(2, 1000)
    with pytest.raises(ValueError, match=r"\(B, n\)"):
        rs(torch.zeros(1000))
    with pytest.raises(ValueError, match="out is"):
        rs(x, out=torch.zeros(2, 362))
    with pytest.raises(ValueError, match="out is"):
        rs(x, out=torch.zeros(3, 400))
    with pytest.raises(ValueError, match="out is"):
        rs(x, out=torch.zeros(2, 400, dtype=torch.float64))
    with pytest.raises(ValueError, match="outputs per row"):
        rs(x, out_len=0)
    with pytest.raises(ValueError, match="per stream|per row"):
        rs(x, lengths=[1, 2, 3])
    with pytest.raises(ValueError, match="length lies in"):
        rs(x, lengths=[5, 1001])
    with pytest.raises(ValueError, match="window is"):
        rs(x, window=(1, 2, 3))
    with pytest.raises(ValueError, match="per stream"):
        rs(x, window=([1, 2, 3], 5))
    taps, first = rs.host_table()
    assert tuple(taps.shape) == (135, 160) and tuple(first.shape) == (160,)


def test_cpu_tensors_fail_loudly(lib):
    from viai_amd import wav_resample as WR
    from viai_amd._lib import ViaiLibraryError
    rs = WR.Resampler(16000, 48000)
    with pytest.raises(ViaiLibraryError, match="GPU only; no CPU fallback"):
        rs(torch.zeros(2, 100))
    with pytest.raises(ViaiLibraryError, match="GPU only; no CPU fallback"):
        rs(torch.zeros(2, 100), lengths=[3, 100], window=(0, 10), out=torch.zeros(2, 300))

    class Front:
        class cfg:
            sample_rate, hop_size, fft_size = 16000, 256, 1024

    class Inpainter:
        front = Front
    with pytest.raises(ViaiLibraryError, match="GPU only; no CPU fallback"):
        WR.inpaint_at_rate(Inpainter, torch.zeros(2, 22272), 48000, [100, 200], [50, 0])
    with pytest.raises(ValueError, match="inside the clip's 22272 samples"):
        WR.inpaint_at_rate(Inpainter, torch.zeros(2, 22272), 48000, [100, 22000], [50, 300])
    with pytest.raises(ValueError, match="positive integer"):
        WR.inpaint_at_rate(Inpainter, torch.zeros(2, 22272), 0, 100, 50)


def test_python_gap_at_rate_is_the_host_rule(lib):
    from viai_amd import wav_resample as WR
    for rates in R.RATIOS:
        rs = WR.Resampler(*rates)
        L, M, H, T = R.RATIOS[rates]
        m = rs.out_len(20400)
        k0, k1 = R.gap_at_rate(5000, 5800, L, M, H, m)
        assert WR.gap_at_rate(5000, 800, rs, m) == (k0, k1 - k0) and k1 - k0 > 800 * L // M
        assert WR.gap_at_rate(5000, 0, rs, m) == (0, 0)
        starts, lens = WR.gap_at_rate([0, 5000, 20000, 7], [10, 800, 400, 0], rs, m)
        want = [R.gap_at_rate(a, a + b, L, M, H, m) for a, b in ((0, 10), (5000, 800), (20000, 400), (7, 0))]
        assert starts == [w[0] for w in want] and lens == [w[1] - w[0] for w in want]
        assert WR.gap_at_rate(torch.tensor([5000, 0]), 800, rs, m)[0][0] == want[1][0]
    with pytest.raises(ValueError, match="one entry per stream"):
        WR.gap_at_rate([1, 2, 3], [4, 5], WR.Resampler(48000, 16000), 100)


def test_the_module_is_reached_by_its_own_name_only():
    import viai_amd
    from viai_amd import wav_resample as WR
    for name in ("Resampler", "gap_at_rate", "inpaint_at_rate"):
        assert callable(getattr(WR, name))
        with pytest.raises(AttributeError):
            getattr(viai_amd, name)
