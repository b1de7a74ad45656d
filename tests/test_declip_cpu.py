"""CPU: the host mirror of the bound-constrained Janssen restoration (`declip_fill_host`, csrc/declip.hip's viai_declip_host) -- consistency with
the bounds, quality against the project's own `janssen_fill_host`, agreement with the numpy restatement of tests/declip_common.py, a mixed
list of dropouts and clip runs, and the refusals.  Needs the built library, not a GPU; the device is compared with this mirror bit for bit in
tests/test_declip_gpu.py.

Tolerance.  max |mirror (fp32) - restatement before its rounding (fp64)| / the row's peak over the solved samples: profiles/declip_rate.json
holds under `tolerance` the worst case measured over `declip_common.tolerance_inputs()` (`measured`, 6.5e-8: the mirror's one rounding to fp32
and a few fp64 units of summation order) and ten times that (`allowed`), which is what is asserted.
Quality.  Set by the issue, not measured from the code: at the defaults the SNR over the clipped samples exceeds `janssen_fill_host(order=32,
context=256, iters=3)` on the same lists by at least 3 dB and exceeds the clipped signal's own; sweeps=3 is not worse than sweeps=1.  Measured:
seed 1: clipped 6.48, janssen_fill 12.23, declip 15.82 (1 sweep) and 24.00 dB (3 sweeps); seed 2: 6.91, 12.53, 16.43 and 24.87 dB; with
rounds=0, sweeps=1, 38 and 43 of the clipped samples come back inside the clipping level."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import ar_fill_common as A
import declip_common as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1                                                                  # hipErrorInvalidValue


@pytest.fixture(scope="module")
def lib():
    from viai_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def profile():
    with open(os.path.join(ROOT, "profiles", "declip_rate.json")) as f:
        return json.load(f)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


_FILLS = {}


def speech_fill(seed, **kw):
    from viai_amd.declip import declip_fill_host
    key = (seed,) + tuple(sorted(kw.items()))
    if key not in _FILLS:
        c = D.speech_case(seed)
        _FILLS[key] = declip_fill_host(c["wav"], c["gaps"], **kw)
    return _FILLS[key]


# ----------------------------------------------------------------------------- 1. the inputs are what the issue describes
@pytest.mark.parametrize("seed", D.SEEDS)
def test_the_speechlike_lists_exercise_capacity_and_cross_cluster_windows(lib, seed):
    from viai_amd.janssen import janssen_plan_host
    c = D.speech_case(seed)
    count, start, length = c["gaps"]
    assert 60 <= int(count[0]) <= 256 and start.shape == (1, 256)
    leader, lo, hi, M = janssen_plan_host(c["wav"].shape[1], c["gaps"], order=32, context=256)
    leaders = sorted(set(leader[0][leader[0] >= 0].tolist()))
    assert len(leaders) >= 3                                                # clusters closed on capacity (248 unknowns at order 32) ...
    assert all(int(M[0, k]) <= 248 for k in leaders)
    ends = [int(start[0, k - 1] + length[0, k - 1]) for k in leaders[1:]]
    assert all(int(start[0, k]) - e < 256 for k, e in zip(leaders[1:], ends))   # ... so every window holds entries of its neighbours
    m, listed = D.clipped_mask(c), D.listed_mask(c["gaps"], c["wav"].shape)
    assert np.all(np.abs(c["wav"][m]) == np.float32(D.CLIP)) and np.all(np.abs(c["wav"][~listed]) < np.float32(D.CLIP))
    assert np.all(np.abs(c["clean"][m]) >= np.float32(D.CLIP)) and 400 <= m.sum() <= listed.sum()


# ----------------------------------------------------------------------------- 2. consistency, exact
@pytest.mark.parametrize("seed", D.SEEDS)
def test_every_solved_sample_satisfies_its_bound_and_nothing_else_changes(lib, seed):
    c = D.speech_case(seed)
    wav = c["wav"]
    for sweeps in (1, 3):
        out, filled = speech_fill(seed, sweeps=sweeps)
        listed = int(c["gaps"][0][0])
        assert (filled[0, :listed] == 1).all() and (filled[0, listed:] == 0).all()
        solved = D.listed_mask(c["gaps"], wav.shape, filled, 1)
        x, cc = out[solved], wav[solved]
        assert out.dtype == np.float32 and np.all(np.sign(cc) * x >= np.abs(cc))          # sign(c) out >= |c| in fp32
        assert D.violations(wav, out, solved) == 0
        assert np.array_equal(bits(out)[~solved], bits(wav)[~solved])                    # every sample outside the lists keeps its bits
    free, _ = speech_fill(seed, rounds=0, sweeps=1)                                      # without the constraint some estimates fall inside
    inside = D.violations(wav, free, D.listed_mask(c["gaps"], wav.shape))
    print("seed %d: %d samples inside the clipping level with rounds=0" % (seed, inside))
    assert inside >= 1


def test_a_long_row_lists_its_two_stretches_and_is_restored_under_its_bounds(lib):
    """declip_common.long_row, 257 tiles of `find_gaps`: what tests/test_declip_gpu.py compares the device with.  The lists fit, their runs lie
    in the two stretches (over a thread edge of the row launch; up to the last sample, alone in its tile), every run is solved, inside its bound"""
    from viai_amd.declip import declip_fill_host
    from viai_amd.gap_detect import find_gaps_host
    wav = D.long_row()
    gaps = find_gaps_host(wav, clip=D.CLIP, min_len=1, max_gaps=D.LONG_MAX_GAPS)
    count = int(gaps.count[0])
    assert 8 <= count <= D.LONG_MAX_GAPS
    start, end = gaps.start[0, :count], gaps.start[0, :count] + gaps.length[0, :count]
    (s0, e0), (s1, e1) = D.LONG_STRETCHES
    first = (start >= s0) & (end <= e0)
    assert np.all(first | ((start >= s1) & (end <= e1))) and 4 <= first.sum() <= count - 4
    assert start[first].min() < 2 * D.LONG_T <= end[first].max() and end.max() == D.LONG_N          # both sides of the edge; the last sample
    out, filled = declip_fill_host(wav, gaps)
    assert (filled[0, :count] == 1).all() and (filled[0, count:] == 0).all()
    solved = D.listed_mask(gaps, wav.shape, filled, 1)
    assert solved.sum() >= count and D.violations(wav, out, solved) == 0
    assert np.array_equal(bits(out)[~solved], bits(wav)[~solved])


# ----------------------------------------------------------------------------- 3. quality against the project's own baseline
@pytest.mark.parametrize("seed", D.SEEDS)
def test_declipping_beats_janssen_fill_by_3_db_on_clipped_voiced_sound(lib, seed):
    from viai_amd.janssen import janssen_fill_host
    c = D.speech_case(seed)
    wav, clean = c["wav"], c["clean"]
    m = D.clipped_mask(c)
    base, _ = janssen_fill_host(wav, c["gaps"], order=32, context=256, iters=3)
    snr_clipped, snr_base = D.snr_db(clean, wav, m), D.snr_db(clean, base, m)
    snr_1, snr_3 = D.snr_db(clean, speech_fill(seed, sweeps=1)[0], m), D.snr_db(clean, speech_fill(seed)[0], m)
    print("seed %d: clipped %.2f dB, janssen_fill %.2f dB, declip 1 sweep %.2f dB, defaults %.2f dB" % (seed, snr_clipped, snr_base, snr_1, snr_3))
    assert snr_3 >= snr_base + 3.0
    assert snr_3 > snr_clipped
    assert snr_3 >= snr_1
    rec = profile()["quality"][D.SEEDS.index(seed)]                                      # the recorded figures are those of this code
    assert rec["declip_snr_db_sweeps3"] == pytest.approx(snr_3, abs=0.006) and rec["janssen_fill_snr_db"] == pytest.approx(snr_base, abs=0.006)


# ----------------------------------------------------------------------------- 4. the numpy restatement
def test_host_mirror_agrees_with_the_numpy_restatement_within_the_recorded_tolerance(lib):
    from viai_amd.declip import declip_fill_host
    tol = profile()["tolerance"]
    assert tol["allowed"] == pytest.approx(10.0 * tol["measured"]) and 0.0 < tol["allowed"] < 1e-5
    worst = D.worst_relative_difference(declip_fill_host)
    print("host mirror against the restatement: %.3e (allowed %.3e)" % (worst, tol["allowed"]))
    assert worst <= tol["allowed"]


def test_the_case_table_gives_the_codes_the_rule_states(lib):
    f = lambda name: D.host(D.case_by_name(name))[1].tolist()
    assert f("M = 1") == [[1]] and f("every sample violates") == [[1]] and f("both row ends") == [[1, 1], [1, 1]]
    assert f("K larger than count") == [[1, 1, 0, 0, 0], [1, 0, 0, 0, 0]]
    assert f("all zero") == [[1, 1]]                                       # a = [1, 0, ...], G the identity: solved, and every bound is 0
    assert f("no model") == [[4]]
    c = D.case_by_name("every sample violates")
    assert np.all(D.host(c)[0][0, 400:420] == np.float32(5.0))              # all pinned at the recorded level: no free unknown, no second solve
    c = D.case_by_name("no model")
    assert np.array_equal(bits(D.host(c)[0]), bits(c["wav"]))               # the start value is written
    c = D.case_by_name("all zero")
    assert not D.host(c)[0].any()
    for name in D.case_names():                                             # consistency over the whole table
        c = D.case_by_name(name)
        out, filled = D.host(c)
        assert D.violations(c["wav"], out, D.listed_mask(c["gaps"], c["wav"].shape, filled, 1)) == 0, name
        untouched = ~D.listed_mask(c["gaps"], c["wav"].shape, filled)
        assert np.array_equal(bits(out)[untouched], bits(c["wav"])[untouched]), name


def test_the_window_is_not_cut_at_other_clusters_and_reads_src_there(lib):
    """two clusters that do not join on capacity (200 + 100 unknowns > 248 at order 32) 40 samples apart: the second one's window reaches into the
    first one's run, so changing the FIRST one's recorded samples changes the second one's result, which janssen_fill's walls do not allow"""
    from viai_amd.declip import declip_fill_host
    from viai_amd.janssen import janssen_fill_host, janssen_plan_host
    clean = A.tones("dc.walls", 1, 1400, 0.01)
    rows = [[(400, 200), (640, 100)]]
    gaps = A.lists(rows, 2)
    assert janssen_plan_host(1400, gaps, order=32, context=64)[0].tolist() == [[0, 1]]
    wav = D.clip_rows(clean, rows, 0.05)
    other = wav.copy()
    other[0, 590:600] *= np.float32(0.5)
    kw = dict(order=32, context=64)
    a, fa = declip_fill_host(wav, gaps, sweeps=1, **kw)
    b, fb = declip_fill_host(other, gaps, sweeps=1, **kw)
    assert fa.tolist() == [[1, 1]] and fb.tolist() == [[1, 1]]
    assert not np.array_equal(a[0, 640:740], b[0, 640:740])
    ja, jb = janssen_fill_host(wav, gaps, **kw)[0], janssen_fill_host(other, gaps, **kw)[0]
    assert np.array_equal(bits(ja[0, 640:740]), bits(jb[0, 640:740]))


# ----------------------------------------------------------------------------- 5. a mixed list
def test_a_mixed_list_solves_dropouts_freely_and_clip_runs_under_their_bounds(lib):
    clean, c = D.clean_mixed()
    out, filled = D.host(c)
    assert filled.tolist() == [[1, 1, 1]]
    from viai_amd.janssen import janssen_plan_host
    assert janssen_plan_host(c["wav"].shape[1], c["gaps"], order=16, context=256)[0].tolist() == [[0, 0, 0]]           # one cluster
    zeros = out[0, 500:540]
    assert np.all(c["wav"][0, 500:540] == 0.0) and np.any(zeros > 0) and np.any(zeros < 0)       # unconstrained: both signs come back
    m = np.zeros(c["wav"].shape, dtype=bool)
    m[0, 500:540] = True
    assert D.snr_db(clean, out, m) > 10.0                                   # and they follow the signal (three sinusoids and a little noise)
    clip = D.listed_mask(c["gaps"], c["wav"].shape) & ~m
    assert clip.sum() == 21 and D.violations(c["wav"], out, clip) == 0
    assert np.all(np.sign(c["wav"][clip]) * out[clip] >= np.abs(c["wav"][clip]))


# ----------------------------------------------------------------------------- 6. refusals
def test_python_refusals_and_exports(lib):
    import viai_amd
    from viai_amd import declip as M
    from viai_amd._lib import ViaiLibraryError
    assert viai_amd.declip_fill is M.declip_fill and viai_amd.declip_fill_host is M.declip_fill_host
    assert viai_amd.declip_file is M.declip_file and callable(viai_amd.declip) and callable(M.declip)
    with pytest.raises(ValueError):
        viai_amd.declip(torch.zeros(1, 64), -1.0)                           # the package attribute (the module, callable) is declip()
    wav = np.zeros((1, 64), dtype=np.float32)
    gaps = A.lists([[(10, 5)]], 1)
    tg = tuple(torch.from_numpy(g) for g in gaps)
    with pytest.raises(ViaiLibraryError):
        M.declip_fill(torch.zeros(1, 64), tg)                               # a CPU tensor: no fallback
    for bad in (dict(rounds=-1), dict(rounds=9), dict(rounds=1.5), dict(sweeps=0), dict(sweeps=17), dict(order=0), dict(order=129),
                dict(context=1), dict(context=1025), dict(iters=0), dict(iters=17), dict(max_len=0), dict(max_len=249),
                dict(order=7, context=1024, max_len=1025), dict(order=128, max_len=64)):
        with pytest.raises(ValueError):
            M.declip_fill_host(wav, gaps, **bad)
        with pytest.raises(ValueError):
            M.declip_fill(torch.zeros(1, 64), tg, **bad)                    # before the device is asked for
    for ok in (dict(rounds=0), dict(rounds=8), dict(sweeps=16), dict(max_len=248), dict(order=128, max_len=63), dict(iters=16), dict(context=2)):
        M.declip_fill_host(wav, gaps, **ok)
    with pytest.raises(ValueError):
        M.declip(torch.zeros(1, 64), 0.0)                                   # clip > 0, before the device is asked for


def test_c_abi_refusals(lib):
    n, K = 100, 4
    ref = np.zeros((1, n), dtype=np.float32)
    src, out = ref.copy(), ref.copy()
    cnt = np.array([1], dtype=np.int32)
    st = np.array([[10, 0, 0, 0]], dtype=np.int32)
    ln = np.array([[5, 0, 0, 0]], dtype=np.int32)
    filled = np.zeros((1, K), dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def args(**kw):
        v = dict(ref=p(ref), src=p(src), lengths=None, stride=n, B=1, n=n, count=p(cnt), start=p(st), length=p(ln), K=K, order=32, context=16,
                 max_len=8, iters=2, rounds=3, out=p(out), out_stride=n, filled=p(filled))
        v.update(kw)
        return [v[k] for k in ("ref", "src", "lengths", "stride", "B", "n", "count", "start", "length", "K", "order", "context", "max_len", "iters",
                               "rounds", "out", "out_stride", "filled")]
    assert lib.viai_declip_host(*args()) == 0 and filled.tolist() == [[1, 0, 0, 0]]
    assert lib.viai_declip_host(*args(src=p(ref))) == 0                                  # src may be ref
    base = out.ctypes.data
    for kw in (dict(out=p(src)), dict(out=p(ref)), dict(src=p(out)),                     # out overlapping src or ref, wholly ...
               dict(src=C.c_void_p(base + 4 * (n - 1))), dict(ref=C.c_void_p(base - 4 * (n - 1))),   # ... or by one sample
               dict(rounds=-1), dict(rounds=9),
               dict(order=0), dict(order=129), dict(context=1), dict(context=1025), dict(iters=0), dict(iters=17), dict(max_len=0),
               dict(context=1024, max_len=249), dict(order=7, context=1024, max_len=1025), dict(order=128, context=1024, max_len=64),
               dict(context=2000), dict(ref=None), dict(src=None), dict(out=None), dict(filled=None), dict(count=None), dict(start=None),
               dict(length=None), dict(B=0), dict(K=0), dict(n=0), dict(n=2 ** 31, stride=2 ** 31, out_stride=2 ** 31), dict(stride=n - 1),
               dict(out_stride=n - 1)):
        assert lib.viai_declip_host(*args(**kw)) == INVALID, kw
    for kw in (dict(rounds=0), dict(rounds=8)):
        assert lib.viai_declip_host(*args(**kw)) == 0, kw
    both = np.zeros((2, n), dtype=np.float32)                                            # adjacent is not overlapping
    assert lib.viai_declip_host(*args(ref=p(both[0]), src=p(both[0]), out=p(both[1]))) == 0
    # the device entry refuses the same before any launch, and wants 4-byte aligned rows
    assert lib.viai_declip(*args(out=p(src)), None) == INVALID
    assert lib.viai_declip(*args(rounds=9), None) == INVALID
    assert lib.viai_declip(*args(src=C.c_void_p(src.ctypes.data + 2)), None) == INVALID
