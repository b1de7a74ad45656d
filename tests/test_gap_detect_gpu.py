"""GPU: `viai_amd.gap_detect.find_gaps` (csrc/gap_detect.hip) equals the numpy statement of the rule EXACTLY -- count, start and length are
integers -- on every case of tests/gap_detect_common.py (T = VIAI_GAP_DETECT_TILE = 4096: runs on sample 0, on n, on tile and word edges, over
whole tiles; the predicate's edge values; ragged rows; merging; overflow; random damage at three densities), and `repair` is the hand-written
sequence of `AudioInpainter` calls.

Sizes: the largest clip of the shared table is 8 T + 5 = 32 773 samples; rows that are 16-byte aligned take the kernel's float4 loads, the others
(odd n, odd strides) its 4-byte loads.

Long rows (`gap_detect_common.long_rows`; the rule is the vectorised `raw_runs_fast`).  Above 256 T = 1 048 576 samples a thread of
gd_rows_kernel owns per = ceil(tiles / 256) > 1 tiles, and its four tile loops, the block scans fed by them, and gd_emit_kernel's tile
indices and `off > K` return far into a row run for the first time:
    test_find_gaps_equals_the_numpy_rule_on_long_rows               n = 256 T + 1 (257 tiles, per 2) and 600 T + 5 (601 tiles, per 3): runs over
                                                                    tile edges inside a thread's range and over thread edges, over several
                                                                    threads' ranges, to the end of the row, the lone last sample, merging
                                                                    across an edge, overflow, ragged lengths, random damage
    test_entries_behind_the_runs_are_written_as_zero_on_long_rows   the two overflow cases on sentinel-filled outputs
    test_a_long_row_alone_is_its_row_in_the_batch                   the ragged case"""
import gc

import numpy as np
import pytest
import torch

import gap_detect_common as G

pytestmark = pytest.mark.gpu

SENTINEL = -77


def bits(t):
    return t.contiguous().view(torch.int32)


def on_device(c):
    """the case's clip as the (B, n) view of its (B, stride) tensor"""
    return torch.from_numpy(c["wav"]).cuda()[:, :c["n"]]


def assert_gaps(got, want, what=""):
    for g, w, name in zip(got, want, ("count", "start", "length")):
        assert g.dtype == torch.int32 and g.is_cuda and tuple(g.shape) == w.shape, (what, name)
        assert np.array_equal(g.cpu().numpy(), w), (what, name, g.cpu().numpy(), w)


# ----------------------------------------------------------------------------- 1. every shared case, exactly
@pytest.mark.parametrize("name", G.case_names())
def test_find_gaps_equals_the_numpy_rule(name):
    from viai_amd.gap_detect import Gaps, find_gaps
    c = G.case_by_name(name)
    wav = on_device(c)
    got = find_gaps(wav, lengths=c["lengths"], **c["kw"])
    assert isinstance(got, Gaps)
    assert_gaps(got, G.expected(c), name)


def test_lengths_may_live_on_the_device():
    from viai_amd.gap_detect import find_gaps
    c = G.case_by_name("ragged stride > n")
    got = find_gaps(on_device(c), lengths=torch.from_numpy(c["lengths"]).cuda(), **c["kw"])
    assert_gaps(got, G.expected(c))


# ----------------------------------------------------------------------------- 2. outputs hold nothing but the answer
@pytest.mark.parametrize("name", ["overflow K=3", "overflow K=1", "overflow K=1 merging", "geometry n=1 min_len=1", "merging within 10"])
def test_entries_behind_the_runs_are_written_as_zero(name):
    """the C call on outputs filled with a sentinel: count is the true number, the first K runs are there, everything behind them is 0"""
    check_sentinel_filled_outputs(G.case_by_name(name), name.startswith("overflow"))


def check_sentinel_filled_outputs(c, overflows):
    from viai_amd import _lib
    from viai_amd.ops import _stream
    name = c["name"]
    wav = on_device(c).contiguous()
    B, n = wav.shape
    kw = dict(threshold=0.0, clip=0.0, merge_within=0)
    kw.update(c["kw"])
    K = kw["max_gaps"]
    lib = _lib.load()
    ws = torch.full(((lib.viai_gap_detect_ws_bytes(B, n, K) + 7) // 8,), -1, dtype=torch.int64, device="cuda")
    count = torch.full((B,), SENTINEL, dtype=torch.int32, device="cuda")
    start = torch.full((B, K), SENTINEL, dtype=torch.int32, device="cuda")
    length = torch.full((B, K), SENTINEL, dtype=torch.int32, device="cuda")
    _lib.check(lib.viai_gap_detect(wav.data_ptr(), None, n, B, n, kw["threshold"], kw["clip"], kw["min_len"], kw["merge_within"], K,
                                   count.data_ptr(), start.data_ptr(), length.data_ptr(), ws.data_ptr(), _stream()), "viai_gap_detect")
    want = G.expected(c)
    assert_gaps((count, start, length), want, name)
    cnt = count.cpu().numpy()
    for b in range(B):
        k = min(int(cnt[b]), K)
        assert int(start[b, k:].abs().sum()) == 0 and int(length[b, k:].abs().sum()) == 0
        assert int((length[b, :k] > 0).sum()) == k
    if overflows:
        assert int(cnt.max()) > K                                         # the case overflows, as its name says


# ----------------------------------------------------------------------------- 2b. rows of more than 256 tiles: a thread of launch 2 walks 2 or 3
@pytest.mark.parametrize("name", G.long_case_names())
def test_find_gaps_equals_the_numpy_rule_on_long_rows(name):
    from viai_amd.gap_detect import find_gaps
    c = G.long_case_by_name(name)
    assert_gaps(find_gaps(on_device(c), lengths=c["lengths"], **c["kw"]), G.expected(c), name)


@pytest.mark.parametrize("per", sorted(G.LONG_N))
def test_entries_behind_the_runs_are_written_as_zero_on_long_rows(per):
    """tiles far behind the K-th run return from launch 3 at once (off > K); with everything merged launch 2 writes the one length"""
    check_sentinel_filled_outputs(G.long_case_by_name("long per=%d overflow K=3" % per), True)
    check_sentinel_filled_outputs(G.long_case_by_name("long per=%d K=1 merging all" % per), False)


@pytest.mark.parametrize("per", sorted(G.LONG_N))
def test_a_long_row_alone_is_its_row_in_the_batch(per):
    from viai_amd.gap_detect import find_gaps
    c = G.long_case_by_name("long per=%d ragged" % per)
    wav = on_device(c)
    whole = find_gaps(wav, lengths=c["lengths"], **c["kw"])
    assert_gaps(whole, G.expected(c))
    for b in range(wav.size(0)):
        alone = find_gaps(wav[b:b + 1], lengths=c["lengths"][b:b + 1], **c["kw"])      # rows 1 ..: 4-byte aligned only, alone or in the batch
        for a, w in zip(alone, whole):
            assert torch.equal(a[0], w[b]), b


# ----------------------------------------------------------------------------- 3. a row alone, a row in a batch, a second call
def test_rows_do_not_depend_on_the_batch_and_calls_repeat():
    from viai_amd.gap_detect import find_gaps
    c = G.case_by_name("merging within 10")
    wav = on_device(c)[:5].contiguous()
    assert wav.size(0) == 5
    lengths = np.array([700, 2 * G.T, c["n"], c["n"], G.T + 3], dtype=np.int32)
    whole = find_gaps(wav, lengths=lengths, **c["kw"])
    again = find_gaps(wav, lengths=lengths, **c["kw"])
    for a, b in zip(whole, again):
        assert torch.equal(a, b)
    assert whole.count.tolist()[:4] == [6, 6, 6, 6]
    for b in range(5):
        alone = find_gaps(wav[b:b + 1].clone(), lengths=lengths[b:b + 1], **c["kw"])
        for a, w in zip(alone, whole):
            assert torch.equal(a[0], w[b]), b
    c = G.case_by_name("random p=0.5 min_len=3 merge=2")
    wav = on_device(c)
    whole = find_gaps(wav, **c["kw"])
    for b in range(wav.size(0)):
        alone = find_gaps(wav[b:b + 1], **c["kw"])                        # rows 1, 2: not 16-byte aligned, alone or in the batch
        for a, w in zip(alone, whole):
            assert torch.equal(a[0], w[b]), b


def test_other_dtypes_and_layouts_are_converted():
    from viai_amd.gap_detect import find_gaps
    c = G.case_by_name("geometry n=%d min_len=4" % (G.T + 1))
    want = G.expected(c)
    wav = on_device(c)
    assert_gaps(find_gaps(wav.double(), **c["kw"]), want)
    assert_gaps(find_gaps(wav.t().contiguous().t(), **c["kw"]), want)     # column-major: a copy with plain rows


# ----------------------------------------------------------------------------- 4. repair
@pytest.fixture(scope="module")
def tiny():
    """the networks live for the module; afterwards they go, and so do the blocks they left in torch's caching allocator"""
    yield G.tiny_inpainter()
    G.release_tiny_inpainter()
    gc.collect()
    torch.cuda.empty_cache()


class Counting:
    def __init__(self, inner):
        self.inner, self.calls = inner, 0

    def __call__(self, *a, **kw):
        self.calls += 1
        return self.inner(*a, **kw)


PLANTED = ([(1000, 301), (4000, 200)], [(2560, 512)])                    # (start, length) per row


def damaged_clip():
    wav = G.tiny_clip(2)
    assert int((wav == 0).sum()) == 0
    hurt = wav.clone()
    for b, gaps in enumerate(PLANTED):
        for s, k in gaps:
            hurt[b, s:s + k] = 0
    return wav, hurt


def test_repair_is_the_hand_written_passes(tiny):
    from viai_amd.gap_detect import repair
    _, hurt = damaged_clip()
    kept = hurt.clone()
    u = [G.tiny_draws(2, G.RECEPTIVE + 512, "gd.p0"), G.tiny_draws(2, G.RECEPTIVE + 200, "gd.p1")]
    counting = Counting(tiny)
    out, gaps = repair(counting, hurt, uniforms=u)
    out = out.clone()
    assert counting.calls == 2 and torch.equal(bits(hurt), bits(kept))    # the input is not written
    # the returned Gaps are the planted intervals
    assert gaps.count.tolist() == [2, 1] and tuple(gaps.start.shape) == (2, 16)
    assert gaps.start[:, :2].tolist() == [[1000, 4000], [2560, 0]] and gaps.length[:, :2].tolist() == [[301, 200], [512, 0]]
    assert int(gaps.start[:, 2:].abs().sum()) == 0 and int(gaps.length[:, 2:].abs().sum()) == 0
    # the two calls written out by hand
    first = tiny(hurt, [1000, 2560], [301, 512], uniforms=u[0], fade=0).clone()
    want = tiny(first, [4000, 0], [200, 0], uniforms=u[1], fade=0)
    assert torch.equal(bits(out), bits(want))
    # every sample outside the detected gaps keeps its bits, and the gaps were regenerated
    inside = torch.zeros_like(hurt, dtype=torch.bool)
    for b, planted in enumerate(PLANTED):
        for s, k in planted:
            inside[b, s:s + k] = True
    assert torch.equal(bits(out)[~inside], bits(hurt)[~inside])
    assert int((out[inside] != 0).sum()) > int(inside.sum()) // 2
    # gaps handed in: nothing is detected again, the same passes run
    given, same = repair(tiny, hurt, gaps=gaps, uniforms=u)
    assert torch.equal(bits(given), bits(out)) and same.count.tolist() == [2, 1]


def test_repair_of_a_clean_clip_runs_no_pass(tiny):
    from viai_amd.gap_detect import repair
    wav, _ = damaged_clip()
    counting = Counting(tiny)
    out, gaps = repair(counting, wav)
    assert counting.calls == 0 and gaps.count.tolist() == [0, 0]
    assert torch.equal(bits(out), bits(wav)) and int(gaps.start.abs().sum()) == 0 and int(gaps.length.abs().sum()) == 0


def test_repair_refuses_an_overflowing_detection(tiny):
    from viai_amd.gap_detect import repair
    _, hurt = damaged_clip()
    kept = hurt.clone()
    counting = Counting(tiny)
    with pytest.raises(ValueError, match=r"rows \[0\]"):
        repair(counting, hurt, max_gaps=1)
    assert counting.calls == 0 and torch.equal(bits(hurt), bits(kept))
