"""The gap-detection rule of include/viai_hip.h restated in numpy, and the cases tests/test_gap_detect_cpu.py and tests/test_gap_detect_gpu.py share.

    damaged(x):  not finite, or |x| <= threshold, or (clip > 0 and |x| >= clip)
    1  raw runs: maximal intervals of damaged samples inside [0, len), len = clamp(lengths[b], 0, n)       a loop over samples
    2  kept: e - s >= min_len                                                                              )
    3  a kept run joins the kept run before it when s - e_prev <= merge_within                             ) a loop over runs
    4  count = all of them; start / length = the first K, zeros behind                                     )

A case is a dict: name, wav (B, stride) float32 with the clip in its first n columns, n, lengths (or None) and the rule's keyword arguments.
`expected(case)` computes the rule once per case and keeps it."""
import numpy as np

T = 4096                                                                  # VIAI_GAP_DETECT_TILE; the CPU test checks it against the header
GOOD = np.float32(0.5)


# ------------------------------------------------------------------------------------------------------------------------------ the rule
def raw_runs(row, length, threshold, clip):
    """step 1, sample by sample: [(s, e)]"""
    threshold, clip = np.float32(threshold), np.float32(clip)
    runs, s = [], None
    for i in range(length):
        x = row[i]
        a = np.abs(x)
        bad = (not np.isfinite(x)) or a <= threshold or (clip > 0 and a >= clip)
        if bad and s is None:
            s = i
        elif not bad and s is not None:
            runs.append((s, i))
            s = None
    if s is not None:
        runs.append((s, length))
    return runs


def merged_runs(runs, min_len, merge_within):
    """steps 2 and 3, run by run"""
    out = []
    for s, e in runs:
        if e - s < min_len:
            continue
        if out and s - out[-1][1] <= merge_within:
            out[-1] = (out[-1][0], e)
        else:
            out.append((s, e))
    return out


def raw_runs_fast(row, length, threshold, clip):
    """step 1 on whole arrays, for rows of millions of samples: the damage mask with the same fp32 comparisons, run edges from the differences
    of the zero-padded mask.  tests/test_gap_detect_cpu.py holds it equal to `raw_runs` on every row of `all_cases()`."""
    threshold, clip = np.float32(threshold), np.float32(clip)
    x = np.asarray(row[:length], dtype=np.float32)
    with np.errstate(invalid="ignore"):
        a = np.abs(x)
        bad = ~np.isfinite(x) | (a <= threshold)
        if clip > 0:
            bad |= a >= clip
    edge = np.diff(np.concatenate(([0], bad.astype(np.int8), [0])))
    return list(zip(np.flatnonzero(edge == 1).tolist(), np.flatnonzero(edge == -1).tolist()))


def rule(wav, n, lengths=None, threshold=0.0, clip=0.0, min_len=64, merge_within=0, max_gaps=16, raw=raw_runs):
    """-> (count (B,), start (B, K), length (B, K)) int32; raw: `raw_runs` or `raw_runs_fast`"""
    B, K = wav.shape[0], max_gaps
    count = np.zeros(B, dtype=np.int32)
    start = np.zeros((B, K), dtype=np.int32)
    length = np.zeros((B, K), dtype=np.int32)
    for b in range(B):
        ln = n if lengths is None else min(max(int(lengths[b]), 0), n)
        runs = merged_runs(raw(wav[b], ln, threshold, clip), min_len, merge_within)
        count[b] = len(runs)
        for k, (s, e) in enumerate(runs[:K]):
            start[b, k], length[b, k] = s, e - s
    return count, start, length


_EXPECTED = {}


def expected(case):
    if case["name"] not in _EXPECTED:
        got = rule(case["wav"], case["n"], case["lengths"], raw=raw_runs_fast if case.get("fast") else raw_runs, **case["kw"])
        for a in got:
            a.setflags(write=False)
        _EXPECTED[case["name"]] = got
    return _EXPECTED[case["name"]]


# ------------------------------------------------------------------------------------------------------------------------------ the cases
def rows_with(n, runs_per_row, pad=0, bad=0.0):
    """(B, n + pad) of good samples (0.5 and -0.5 in turn) with `bad` written into every [s, e) of a row's list; the pad is damaged"""
    B = len(runs_per_row)
    wav = np.tile(np.where(np.arange(n + pad) % 2 == 0, GOOD, -GOOD).astype(np.float32), (B, 1))
    for b, runs in enumerate(runs_per_row):
        for s, e in runs:
            assert 0 <= s <= e <= n, (s, e, n)
            wav[b, s:e] = bad
    wav[:, n:] = 0.0
    return wav


def case(name, wav, n=None, lengths=None, **kw):
    kw.setdefault("min_len", 4)
    kw.setdefault("max_gaps", 16)
    return {"name": name, "wav": wav, "n": wav.shape[1] if n is None else n, "lengths": lengths, "kw": kw}


def geometry_rows(n):
    """the run patterns of the issue that fit n samples, one row each (min_len 4: runs of 3 are dropped, of 4 kept)"""
    rows = [[(0, min(n, 6))],                                             # starts at sample 0
            [(max(0, n - 6), n)],                                         # ends at n
            [(0, n)],                                                     # the whole row
            []]                                                           # none at all
    if n >= 32:
        rows.append([(8, 11), (20, 24)])                                  # min_len - 1 (dropped) and min_len (kept)
        rows.append([(1, 5), (n - 5, n - 1)])                             # one good sample at either end
    if n > 64:
        rows.append([(60, min(n, 70))])                                   # crosses a 64-sample word edge
    if n >= T:
        rows.append([(T - 9, T)])                                         # ends exactly on a tile edge
        rows.append([(T - 64, T), (10, 20)])                              # ... and on a word edge too
    if n > T:
        rows.append([(T, n)])                                             # starts exactly on a tile edge (one sample at n = T + 1)
        rows.append([(T - 1, n)])                                         # crosses it by one sample
    if n >= 3 * T + 17:
        rows.append([(T, T + 9), (2 * T - 9, 2 * T), (3 * T, 3 * T + 4)])           # starts and ends on tile edges
        rows.append([(T - 3, 3 * T + 5)])                                           # two whole tiles and more
        rows.append([(5, 3 * T + 17)])                                              # three tiles to the end of the row
        rows.append([(0, 2 * T), (2 * T + 1, 3 * T)])                               # whole tiles, one good sample between
        rows.append([(T - 2, T + 2), (T + 3, T + 6), (2 * T - 4, 2 * T), (2 * T + 1, 2 * T + 5), (3 * T + 13, 3 * T + 17)])
    return rows


GEOMETRY_N = (1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17)


def geometry_cases():
    out = []
    for n in GEOMETRY_N:
        wav = rows_with(n, geometry_rows(n))
        out.append(case("geometry n=%d min_len=4" % n, wav))
        out.append(case("geometry n=%d min_len=1" % n, wav, min_len=1))
        out.append(case("geometry n=%d min_len=4 merge=1" % n, wav, merge_within=1))
    return out


def predicate_cases():
    n = 96
    f = np.float32
    thr, clp = f(0.1), f(0.9)
    above, below = np.nextafter(thr, f(1)), np.nextafter(clp, f(0))
    special = [f("nan"), f("inf"), f("-inf"), f(-0.0), f(0.0), f(1e-40), -f(1e-40), thr, -thr, above, -above, clp, -clp, below, -below, f(1.5),
               f(1e30), f(-3e38), f(1e-30)]
    assert special[5] != 0 and special[5] < np.finfo(np.float32).tiny        # a denormal that survived
    wav = rows_with(n, [[]])
    for j, v in enumerate(special):                                          # isolated: a good sample on either side
        wav[0, 3 + 4 * j] = v
    wav[0, 90:94] = f("nan")                                                 # and a run of mixed non-finite values
    wav[0, 91] = f("-inf")
    kw = dict(min_len=1, max_gaps=32)
    return [case("predicate zeros only", wav, **kw),
            case("predicate threshold", wav, threshold=float(thr), **kw),
            case("predicate clip", wav, clip=float(clp), **kw),
            case("predicate threshold and clip", wav, threshold=float(thr), clip=float(clp), **kw),
            case("predicate threshold denormal", wav, threshold=1e-40, **kw),
            case("predicate clip off large samples", wav, clip=0.0, **kw),
            case("predicate threshold inf", wav, threshold=float("inf"), **kw),
            case("predicate clip inf", wav, clip=float("inf"), **kw)]


def ragged_cases():
    n, pad = T + 100, 5
    runs = [(10, 30), (T - 10, T + 20), (T + 50, T + 100)]
    wav = rows_with(n, [runs] * 7, pad=pad)
    lengths = np.array([0, T + 5, n + 50, T + 40, -3, T, n], dtype=np.int32)    # nothing; inside a run; above n; damage beyond len; negative
    return [case("ragged stride > n", wav, n=n, lengths=lengths),
            case("ragged stride > n, no lengths", wav, n=n),
            case("ragged stride = n", np.ascontiguousarray(wav[:, :n]), lengths=lengths)]


def merging_cases():
    base = [(100, 110), (120, 130), (141, 150),                              # distance 10 joins, 11 does not
            (300, 310), (315, 325), (330, 340),                              # a chain of three
            (500, 510), (512, 514), (520, 530),                              # kept, dropped, kept: 10 from kept to kept, joins
            (600, 610), (613, 615), (621, 630)]                              # ... 11 from kept to kept: does not, whatever the dropped run is near
    n = 2 * T + 50
    rows = [base] + [[(s + d, e + d) for s, e in base] for d in (T - 505, T - 125, T - 335, 2 * T - 615, T - 100)]
    rows.append([(T - 20, T - 10), (T, T + 10), (2 * T - 4, 2 * T + 4), (2 * T + 14, 2 * T + 18)])
    wav = rows_with(n, rows)
    return [case("merging within 10", wav, merge_within=10),
            case("merging within 0", wav, merge_within=0),
            case("merging within 10 min_len 1", wav, merge_within=10, min_len=1),
            case("merging everything", wav, merge_within=n)]


def overflow_cases():
    n = T + 300
    rows = [[(100 * (k // 2) + 40 * (k % 2), 100 * (k // 2) + 40 * (k % 2) + 10) for k in range(10)],     # ten runs in one tile, 30 and 50 apart in turn
            [(T - 100 + 40 * k, T - 100 + 40 * k + 10) for k in range(9)],    # nine across the tile edge
            [(7, 17)], []]
    wav = rows_with(n, rows)
    return [case("overflow K=3", wav, max_gaps=3),
            case("overflow K=1", wav, max_gaps=1),
            case("overflow K=9", wav, max_gaps=9),
            case("overflow K=1 merging", wav, max_gaps=1, merge_within=30),
            case("overflow K=2 merging all", wav, max_gaps=2, merge_within=n)]


RANDOM_P = (0.02, 0.5, 0.98)
RANDOM_RULES = ((1, 0), (3, 2), (8, 20), (64, 100))


def random_cases():
    n, B = 8 * T + 5, 3
    out = []
    for j, p in enumerate(RANDOM_P):
        g = np.random.default_rng(20 + j)
        wav = g.uniform(0.1, 0.9, size=(B, n)).astype(np.float32)
        wav[g.random((B, n)) < p] = 0.0
        for min_len, merge_within in RANDOM_RULES:
            out.append(case("random p=%g min_len=%d merge=%d" % (p, min_len, merge_within), wav, min_len=min_len, merge_within=merge_within,
                            max_gaps=64))
    return out


_CASES = []


def all_cases():
    if not _CASES:
        _CASES.extend(geometry_cases() + predicate_cases() + ragged_cases() + merging_cases() + overflow_cases() + random_cases())
        assert len({c["name"] for c in _CASES}) == len(_CASES)
    return _CASES


def case_names():
    return [c["name"] for c in all_cases()]


def case_by_name(name):
    return next(c for c in all_cases() if c["name"] == name)


# ------------------------------------------------------------------------------------------------------------------------------ long rows
# gd_rows_kernel gives thread k of its 256 the tiles [k per, (k + 1) per), per = ceil(tiles / 256): above 256 T samples a thread walks more than
# one tile.  Two lengths: 257 tiles (per 2: thread 128 owns one tile of one sample, threads 129 .. 255 none) and 601 tiles (per 3: thread 200
# owns one tile of 5 samples).  Both are odd, so every row behind the first takes the 4-byte loads.  E = per T is a "thread edge".
# The rule is `raw_runs_fast`; a group's rows are built when one of its cases is asked for, and only the last group is kept (60 MB at the most).
ROWS_THREADS = 256                                                        # GD_THREADS
LONG_N = {2: 256 * T + 1, 3: 600 * T + 5}
LONG_RANDOM_P = (0.02, 0.5)


def long_rows(group):
    kind, per = group[0], group[1]
    n, E = LONG_N[per], per * T
    L = (n - 1) // T * T                                                  # where the last tile starts
    if kind == "geometry":
        return rows_with(n, [[(E + T - 3, E + T + 3)],                    # across a tile edge inside thread 1's range
                             [(E - 3, E + 3)],                            # across a thread edge
                             [(E + T - 5, 5 * E + T + 7)],                # over several threads' whole ranges (3 T - 5 .. 11 T + 7 at per 2)
                             [(0, n)],                                    # the whole row
                             [(100 * T + 9, n)],                          # from the middle to the end: no good sample behind, the run ends at len
                             [(n - 1, n)]])                               # the lone last sample (kept with min_len 1 only)
    if kind == "merging":
        return rows_with(n, [[(E - 13, E - 3), (E + 3, E + 13)],          # two kept runs 6 apart facing each other across a thread edge
                             [(2 * E - 16, 2 * E - 4), (2 * E - 2, 2 * E + 1), (2 * E + 2, 2 * E + 12)],     # kept, dropped (on the edge), kept: 6
                             [(E + T - 13, E + T - 3), (E + T + 3, E + T + 13)]])      # the pair across a tile edge inside thread 1's range
    if kind == "overflow":
        far = (n // T) // 10 * T                                          # ten runs 25 tiles apart (60 at per 3): later tiles have off > K
        return rows_with(n, [[(k * far + 17 * k + 100, k * far + 17 * k + 110) for k in range(10)],
                             [(j * E - 5, j * E + 5) for j in range(3, 3 + 10 * 12, 12)]])       # ten runs on thread edges
    if kind == "ragged":
        runs = [(E - 6, E + 6), (5 * E, 5 * E + 9), (L - 4, n)]           # on a thread edge, from one, into the last tile
        return rows_with(n, [runs] * 5)
    assert kind == "random"
    g = np.random.default_rng(1000 * per + int(100 * group[2]))
    wav = g.uniform(0.1, 0.9, size=(2, n)).astype(np.float32)
    wav[g.random((2, n)) < group[2]] = 0.0
    return wav


def _long_table():
    out = []
    for per, n in sorted(LONG_N.items()):
        E, L, tag = per * T, (n - 1) // T * T, "long per=%d " % per
        out.append((tag + "geometry min_len=4", ("geometry", per), None, {}))
        out.append((tag + "geometry min_len=1", ("geometry", per), None, dict(min_len=1)))
        out.append((tag + "merging within 6", ("merging", per), None, dict(merge_within=6)))
        out.append((tag + "merging within 5", ("merging", per), None, dict(merge_within=5)))
        out.append((tag + "overflow K=3", ("overflow", per), None, dict(max_gaps=3)))
        out.append((tag + "K=1 merging all", ("overflow", per), None, dict(max_gaps=1, merge_within=n)))
        out.append((tag + "ragged", ("ragged", per), np.array([0, E, L + 1, n + 50, -3], dtype=np.int32), {}))
        for p in LONG_RANDOM_P:
            for min_len, merge_within in RANDOM_RULES:
                out.append((tag + "random p=%g min_len=%d merge=%d" % (p, min_len, merge_within), ("random", per, p), None,
                            dict(min_len=min_len, merge_within=merge_within, max_gaps=64)))
    assert len({r[0] for r in out}) == len(out)
    return out


_LONG_TABLE = _long_table()
_LONG_ROWS = {}


def long_case_names():
    return [r[0] for r in _LONG_TABLE]


def long_case_by_name(name):
    """the case, its rule the vectorised one; the rows of its group are shared with the group's other cases and must not be written"""
    _, group, lengths, kw = next(r for r in _LONG_TABLE if r[0] == name)
    if group not in _LONG_ROWS:
        _LONG_ROWS.clear()
        _LONG_ROWS[group] = long_rows(group)
    c = case(name, _LONG_ROWS[group], lengths=lengths, **kw)
    assert c["wav"].shape[0] <= 8
    c["fast"] = True
    return c


# ------------------------------------------------------------------------------------------------------------------------------ repair()
# A tiny generator and vocoder, built as tests/test_inpaint_audio_gpu.py builds them: 68 mel bands (the smallest legal generator that is a multiple
# of 4), clips of 29 hops = 32 frames, a 4-layer mixture-of-logistics vocoder with receptive field 13.
NUM_MELS, FFT, HOP = 68, 1024, 256
N_CLIP = 29 * HOP
FRAMES = 32
RECEPTIVE = 13
_NETS = {}


def tiny_inpainter():
    import torch  # noqa: F401
    from oracle import viai_oracle as O
    from oracle import wavenet_oracle as W
    if "inp" not in _NETS:
        from viai_amd import AudioInpainter
        from viai_amd.audio import AudioConfig, MelFrontEnd
        from viai_amd.model import AudioModel, StepConfig
        from viai_amd.wavenet import WaveNet

        class Voc(W.WNConfig):
            layers = 4
            stacks = 2
            residual_channels = 32
            gate_channels = 32
            skip_out_channels = 32
            cin_channels = NUM_MELS
            upsample_scales = (4, 4, 4, 4)

        class Cfg(AudioConfig):
            num_mels = NUM_MELS
        net = WaveNet(out_channels=Voc.out_channels, layers=Voc.layers, stacks=Voc.stacks, residual_channels=Voc.residual_channels,
                      gate_channels=Voc.gate_channels, skip_out_channels=Voc.skip_out_channels, kernel_size=3, dropout=0.0,
                      cin_channels=Voc.cin_channels, weight_normalization=True, upsample_scales=list(Voc.upsample_scales), scalar_input=True)
        net.load_state_dict(W.wavenet_state(Voc, "IA."))
        assert net.receptive_field == RECEPTIVE
        hp = StepConfig()
        hp.cin_channels, hp.max_mel_lengths = NUM_MELS, FRAMES
        model = AudioModel(hp, device="cuda:0")
        model.load_states(O.encoder_state(), O.decoder_state(), O.disc_state())
        _NETS["inp"] = AudioInpainter(model, net.cuda().eval(), MelFrontEnd(Cfg, device="cuda:0"))
    return _NETS["inp"]


def release_tiny_inpainter():
    _NETS.clear()


def tiny_clip(B, tag="gd.wav"):
    from oracle import viai_oracle as O
    return O.cf_uniform(tag, (8, N_CLIP), -0.9, 0.9)[:B].contiguous().cuda()


def tiny_draws(B, L, tag):
    """the mixture-of-logistics sampler's uniforms in window coordinates"""
    from oracle import viai_oracle as O
    return (O.cf_uniform(tag + ".u1", (8, L, 10), 1e-5, 1 - 1e-5)[:B].contiguous().cuda(),
            O.cf_uniform(tag + ".u2", (8, L), 1e-5, 1 - 1e-5)[:B].contiguous().cuda())
