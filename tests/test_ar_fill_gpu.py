"""GPU: `viai_amd.ar_fill.ar_fill` (csrc/ar_fill.hip) equals its host mirror BIT FOR BIT, `out` and `filled`, over the table of
tests/ar_fill_common.py; it repeats, and a row alone is the row in a batch; it reads `find_gaps`'s tensors where they lie; and `repair` /
`repair_file` hand the short gaps to it and only the long ones to the inpainter.  The largest clip is 8192 samples."""
import types

import numpy as np
import pytest
import torch

import ar_fill_common as A

pytestmark = pytest.mark.gpu


def bits(t):
    return t.contiguous().view(torch.int32)


def np_bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def dev_gaps(c):
    return tuple(torch.from_numpy(np.ascontiguousarray(g)).cuda() for g in c["gaps"])


def on_device(c):
    return torch.from_numpy(c["wav"]).cuda()[:, :c["n"]]


_HOST = {}


def host(c):
    """the host mirror's answer, computed once per case"""
    from viai_amd.ar_fill import ar_fill_host
    if c["name"] not in _HOST:
        _HOST[c["name"]] = ar_fill_host(c["wav"][:, :c["n"]], c["gaps"], lengths=c["lengths"], **c["kw"])
    return _HOST[c["name"]]


# ----------------------------------------------------------------------------- 1. the device is the host mirror
@pytest.mark.parametrize("name", A.case_names())
def test_device_equals_the_host_mirror_bit_for_bit(name):
    from viai_amd.ar_fill import ar_fill
    c = A.case_by_name(name)
    want, want_filled = host(c)
    wav = on_device(c)
    kept = wav.clone()
    out, filled = ar_fill(wav, dev_gaps(c), lengths=c["lengths"], **c["kw"])
    assert out.is_cuda and out.dtype == torch.float32 and filled.dtype == torch.int32 and tuple(filled.shape) == want_filled.shape
    assert np.array_equal(filled.cpu().numpy(), want_filled), (filled.cpu().numpy(), want_filled)
    assert np.array_equal(bits(out).cpu().numpy(), np_bits(want))
    assert torch.equal(bits(wav), bits(kept))                             # the input is not written
    again, filled2 = ar_fill(wav, dev_gaps(c), lengths=c["lengths"], **c["kw"])
    assert torch.equal(bits(again), bits(out)) and torch.equal(filled2, filled)


@pytest.mark.parametrize("name", ["three gaps a row", "ragged rows", "neighbours", "order 128 context 4096"])
def test_separate_and_aliased_outputs_agree(name):
    """the C call with out a different buffer (wider rows, a sentinel behind them) and with out == wav"""
    from viai_amd import _lib
    from viai_amd.ops import _stream
    c = A.case_by_name(name)
    want, want_filled = host(c)
    lib = _lib.load()
    wav = torch.from_numpy(c["wav"]).cuda()
    B, stride = wav.shape
    n = c["n"]
    count, start, length = dev_gaps(c)
    K = start.size(1)
    lengths = None if c["lengths"] is None else torch.from_numpy(c["lengths"]).cuda()
    lp = 0 if lengths is None else lengths.data_ptr()
    kw = c["kw"]
    out = torch.full((B, n + 3), -77.0, device="cuda")
    out[:, :n] = wav[:, :n]
    filled = torch.full((B, K), -77, dtype=torch.int32, device="cuda")
    _lib.check(lib.viai_ar_fill(wav.data_ptr(), lp, stride, B, n, count.data_ptr(), start.data_ptr(), length.data_ptr(), K, kw["order"],
                                kw["context"], kw["max_len"], out.data_ptr(), n + 3, filled.data_ptr(), _stream()), "viai_ar_fill")
    assert np.array_equal(bits(out[:, :n]).cpu().numpy(), np_bits(want)) and bool((out[:, n:] == -77.0).all())
    assert np.array_equal(filled.cpu().numpy(), want_filled)
    alias = wav.clone()
    _lib.check(lib.viai_ar_fill(alias.data_ptr(), lp, stride, B, n, count.data_ptr(), start.data_ptr(), length.data_ptr(), K, kw["order"],
                                kw["context"], kw["max_len"], alias.data_ptr(), stride, filled.data_ptr(), _stream()), "viai_ar_fill")
    assert np.array_equal(bits(alias[:, :n]).cpu().numpy(), np_bits(want))
    assert torch.equal(bits(alias[:, n:]), bits(wav[:, n:]))


def test_a_row_alone_is_the_row_in_a_batch_of_three():
    from viai_amd.ar_fill import ar_fill
    c = A.case_by_name("three gaps a row")
    wav, gaps = on_device(c), dev_gaps(c)
    whole, filled = ar_fill(wav, gaps, **c["kw"])
    assert wav.size(0) == 3
    for b in range(3):
        alone, f1 = ar_fill(wav[b:b + 1], tuple(g[b:b + 1] for g in gaps), **c["kw"])
        assert torch.equal(bits(alone[0]), bits(whole[b])) and torch.equal(f1[0], filled[b]), b


# ----------------------------------------------------------------------------- 2. find_gaps -> ar_fill, the lists left on the device
B_CLIP, N_CLIP = 3, 5000                                                  # not a whole number of hops
SILENCED = ((700, 64), (2100, 100), (3800, 160))


def damaged_batch(extra=()):
    from viai_amd import synth
    clean = synth.waveform(B_CLIP, N_CLIP, tag="ar.gpu").cuda()
    assert int((clean == 0).sum()) == 0
    hurt = clean.clone()
    for b in range(B_CLIP):
        for s, L in SILENCED + tuple(extra):
            hurt[b, s + 11 * b:s + 11 * b + L] = 0
    return clean, hurt


def test_find_gaps_then_ar_fill_on_the_device():
    from viai_amd.ar_fill import ar_fill
    from viai_amd.gap_detect import find_gaps
    clean, hurt = damaged_batch()
    gaps = find_gaps(hurt)
    ptrs = [g.data_ptr() for g in gaps]
    out, filled = ar_fill(hurt, gaps)
    assert [g.data_ptr() for g in gaps] == ptrs and all(g.is_cuda for g in gaps)
    assert gaps.count.tolist() == [3] * B_CLIP and filled[:, :3].tolist() == [[1, 1, 1]] * B_CLIP and int(filled[:, 3:].abs().sum()) == 0
    host_gaps = tuple(g.cpu().numpy() for g in gaps)
    want, _ = A.fill_rule(hurt.cpu().numpy(), N_CLIP, host_gaps)
    got, ref = out.cpu().numpy(), clean.cpu().numpy()
    inside = torch.zeros_like(hurt, dtype=torch.bool)
    for b in range(B_CLIP):
        spans = [(s + 11 * b, s + 11 * b + L) for s, L in SILENCED]
        for s, e in spans:
            inside[b, s:e] = True
        mine, rule = A.gap_snr_db(ref[b], got[b], spans), A.gap_snr_db(ref[b], want[b], spans)
        print("row %d: gap SNR %.2f dB, restatement %.2f dB" % (b, mine, rule))
        assert abs(mine - rule) <= 1.0
    assert torch.equal(bits(out)[~inside], bits(hurt)[~inside])


# ----------------------------------------------------------------------------- 3. repair
RATE, HOP = 16000, 256


class StubInpainter:
    """called like an AudioInpainter; notes (gap_start, gap_len) and a copy of its input, and returns the input"""
    front = types.SimpleNamespace(cfg=types.SimpleNamespace(sample_rate=RATE, hop_size=HOP))

    def __init__(self):
        self.calls, self.inputs = [], []

    def __call__(self, wav, gap_start, gap_len, video=None, flow=None, uniforms=None, fade=0, return_parts=False):
        self.calls.append(([int(v) for v in gap_start], [int(v) for v in gap_len]))
        self.inputs.append(wav.clone())
        return wav


def test_repair_without_an_inpainter_is_ar_fill():
    from viai_amd.ar_fill import ar_fill
    from viai_amd.gap_detect import find_gaps, repair
    _, hurt = damaged_batch()
    kept = hurt.clone()
    out, gaps = repair(None, hurt, ar_below=256)
    want, _ = ar_fill(hurt, find_gaps(hurt), max_len=255)
    assert torch.equal(bits(out), bits(want)) and gaps.count.tolist() == [3] * B_CLIP and torch.equal(bits(hurt), bits(kept))
    assert not torch.equal(bits(out), bits(hurt))
    _, longer = damaged_batch(extra=((3000, 300),))
    with pytest.raises(ValueError, match=r"rows \[0, 1, 2\].*300"):
        repair(None, longer, ar_below=256)
    with pytest.raises(ValueError, match="no inpainter"):
        repair(None, hurt)                                                # ar_below = 0: every gap is the inpainter's


def test_repair_sends_only_the_long_gaps_to_the_inpainter():
    from viai_amd.ar_fill import ar_fill
    from viai_amd.gap_detect import find_gaps, repair
    wav = torch.rand(2, 4 * HOP * 5, device="cuda") * 0.8 + 0.1
    planted = ([(300, 100), (900, 400), (2000, 64), (3000, 300)], [(500, 64), (1500, 500)])
    for b, runs in enumerate(planted):
        for s, L in runs:
            wav[b, s:s + L] = 0
    stub = StubInpainter()
    out, gaps = repair(stub, wav, ar_below=256)
    assert gaps.count.tolist() == [4, 2]                                  # the detection is returned whole
    assert stub.calls == [([900, 1500], [400, 500]), ([3000, 0], [300, 0])]         # compacted to the front, in order; the short ones never arrive
    filled_first, filled = ar_fill(wav, find_gaps(wav), max_len=255)
    assert filled[:, :4].tolist() == [[1, 0, 1, 0], [1, 0, 0, 0]]
    assert torch.equal(bits(stub.inputs[0]), bits(filled_first)) and torch.equal(bits(out), bits(filled_first))
    assert bool((out[0, 300:400] != 0).all()) and bool((out[0, 900:1300] == 0).all())
    # ar_below = 0: exactly what the stub sees today
    plain = StubInpainter()
    out0, _ = repair(plain, wav)
    assert plain.calls == [([300, 500], [100, 64]), ([900, 1500], [400, 500]), ([2000, 0], [64, 0]), ([3000, 0], [300, 0])]
    assert all(torch.equal(bits(x), bits(wav)) for x in plain.inputs) and torch.equal(bits(out0), bits(wav))


def test_repair_file_with_ar_below(tmp_path):
    import wav_io_common as W
    from viai_amd import wav_io as wio
    n = 5 * HOP + 77
    t = np.arange(n) / RATE
    clean = (0.4 * np.sin(2 * np.pi * 440.0 * t) + 0.3 * np.sin(2 * np.pi * 1234.0 * t + 1.0)).astype(np.float32)
    clean[np.abs(clean) < 1e-3] = 1e-3                                    # no natural zero in the 16-bit file
    runs = [(300, 400), (n - 150, n)]
    hurt = clean.copy()
    for s, e in runs:
        hurt[s:e] = 0
    data = W.encode_rule(hurt[None, :], "s16").tobytes()
    buf = W.wav_file("s16", 1, RATE, data)
    src, dst = str(tmp_path / "src.wav"), str(tmp_path / "dst.wav")
    open(src, "wb").write(buf)
    stub = StubInpainter()
    gaps, info = wio.repair_file(stub, src, dst, ar_below=256)
    assert stub.calls == [] and gaps.count.tolist() == [1 + 1] and gaps.start[0, :2].tolist() == [300, n - 150]
    out = open(dst, "rb").read()
    off = info.data_offset
    assert len(out) == len(buf) and out[:off] == buf[:off] and out[off + info.data_bytes:] == buf[off + info.data_bytes:]
    got = np.frombuffer(out, dtype="<i2", count=n, offset=off)
    old = np.frombuffer(data, dtype="<i2")
    inside = np.zeros(n, dtype=bool)
    for s, e in runs:
        inside[s:e] = True
    assert np.array_equal(got[~inside], old[~inside]) and (got[inside] != old[inside]).mean() > 0.9
    # the fill follows the tones: the gap at the file's end is a forward prediction alone, never pulled to the zero padding behind it
    want = np.frombuffer(W.encode_rule(clean[None, :], "s16").tobytes(), dtype="<i2").astype(np.float64)
    err = got[inside].astype(np.float64) - want[inside]
    assert 10 * np.log10(np.sum(want[inside] ** 2) / np.sum(err ** 2)) > 20.0
