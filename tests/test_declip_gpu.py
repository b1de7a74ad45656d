"""GPU: `declip_fill` (csrc/declip.hip) against its host mirror BIT FOR BIT, on `out` and on `filled`: the case table of tests/declip_common.py
(M = 1; every sample pinned, so no second solve; 300 unknowns compacted across all four waves; order 80; windows cut by both row ends; K
larger than count; an all-zero window; no model; a long noiseless run; a mixed list), the 3-cluster speech-like rows at 1, 2 and 3 sweeps, a
row alone against the same row inside a batch of 8; then `declip` against `find_gaps` + `declip_fill`, `declip` on a row of 256 * 4096 + 1
samples against the host mirrors (test_declip_of_a_long_row_equals_the_host_mirrors: 257 tiles of `find_gaps`), and `declip_file` on a 16-bit file.
The mirror itself is pinned to the numpy restatement by tests/test_declip_cpu.py."""
import numpy as np
import pytest
import torch

import declip_common as D

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def dev_lists(gaps):
    return tuple(torch.from_numpy(np.array(g, dtype=np.int32, order="C", copy=True)).cuda() for g in gaps)


@pytest.mark.parametrize("name", D.case_names())
def test_device_equals_the_host_mirror_bit_for_bit(name):
    from viai_amd.declip import declip_fill
    c = D.case_by_name(name)
    want, want_filled = D.host(c)
    wav = torch.from_numpy(np.ascontiguousarray(c["wav"])).cuda()
    before = wav.clone()
    out, filled = declip_fill(wav, dev_lists(c["gaps"]), lengths=c["lengths"], **c["kw"])      # the lists are read where they lie
    assert out.dtype == torch.float32 and filled.dtype == torch.int32 and out.is_cuda and filled.is_cuda
    assert np.array_equal(filled.cpu().numpy(), want_filled), (filled.cpu().numpy(), want_filled)
    assert np.array_equal(bits(out.cpu().numpy()), bits(want))
    assert torch.equal(wav.view(torch.int32), before.view(torch.int32))                         # the input is not written
    out2, filled2 = declip_fill(wav, c["gaps"], lengths=None if c["lengths"] is None else c["lengths"].tolist(), **c["kw"])   # host lists
    assert torch.equal(out2.view(torch.int32), out.view(torch.int32)) and torch.equal(filled2, filled)


@pytest.mark.parametrize("sweeps", [1, 2, 3])
@pytest.mark.parametrize("seed", D.SEEDS)
def test_speechlike_rows_equal_the_host_mirror_at_every_sweep_count(seed, sweeps):
    from viai_amd.declip import declip_fill, declip_fill_host
    c = D.speech_case(seed)
    want, want_filled = declip_fill_host(c["wav"], c["gaps"], sweeps=sweeps)
    out, filled = declip_fill(torch.from_numpy(c["wav"].copy()).cuda(), dev_lists(c["gaps"]), sweeps=sweeps)
    assert np.array_equal(filled.cpu().numpy(), want_filled)
    assert np.array_equal(bits(out.cpu().numpy()), bits(want))
    solved = D.listed_mask(c["gaps"], c["wav"].shape, want_filled, 1)
    assert D.violations(c["wav"], out.cpu().numpy(), solved) == 0


def test_rounds_0_is_the_unconstrained_solve_on_the_device_too():
    from viai_amd.declip import declip_fill, declip_fill_host
    c = D.speech_case(1)
    want, want_filled = declip_fill_host(c["wav"], c["gaps"], rounds=0, sweeps=1)
    out, filled = declip_fill(torch.from_numpy(c["wav"].copy()).cuda(), dev_lists(c["gaps"]), rounds=0, sweeps=1)
    assert np.array_equal(filled.cpu().numpy(), want_filled) and np.array_equal(bits(out.cpu().numpy()), bits(want))


def test_a_row_alone_is_row_5_of_a_batch_of_8_with_other_neighbours():
    from viai_amd.declip import declip_fill, declip_fill_host
    from viai_amd.gap_detect import find_gaps_host
    rows = np.stack([D.speechlike(20 + b, n=1536)[1] for b in range(8)])
    gaps = find_gaps_host(rows, clip=D.CLIP, min_len=1, max_gaps=128)
    assert int(gaps.count.max()) <= 128 and int(gaps.count.min()) >= 20
    lengths = np.array([1536, 1500, 1536, 1400, 1536, 1511, 1536, 900], dtype=np.int32)
    wav, g, ln = torch.from_numpy(rows).cuda(), dev_lists(gaps), torch.from_numpy(lengths).cuda()
    whole, filled = declip_fill(wav, g, lengths=ln, sweeps=2)
    again, filled2 = declip_fill(wav, g, lengths=ln, sweeps=2)
    assert torch.equal(whole.view(torch.int32), again.view(torch.int32)) and torch.equal(filled, filled2)
    alone, f1 = declip_fill(wav[5:6], tuple(x[5:6] for x in g), lengths=ln[5:6], sweeps=2)
    assert torch.equal(alone[0].view(torch.int32), whole[5].view(torch.int32)) and torch.equal(f1[0], filled[5])
    want, want_filled = declip_fill_host(rows, gaps, lengths=lengths, sweeps=2)
    assert np.array_equal(filled.cpu().numpy(), want_filled) and np.array_equal(bits(whole.cpu().numpy()), bits(want))
    assert (want_filled[7] == 0).any() and (want_filled == 1).any()                            # runs behind a row's length are skipped


def test_declip_is_find_gaps_then_declip_fill_with_the_lists_on_the_device():
    from viai_amd.declip import declip, declip_fill
    from viai_amd.gap_detect import find_gaps
    c = D.speech_case(2)
    wav = torch.from_numpy(c["wav"].copy()).cuda()
    out, gaps, filled = declip(wav, D.CLIP, max_gaps=256, sweeps=2)
    assert all(t.is_cuda for t in gaps) and filled.is_cuda
    ref_gaps = find_gaps(wav, threshold=0.0, clip=D.CLIP, min_len=1, max_gaps=256)
    assert all(torch.equal(a, b) for a, b in zip(gaps, ref_gaps))
    assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(gaps, c["gaps"]))             # and those are the host's lists
    ref, ref_filled = declip_fill(wav, ref_gaps, sweeps=2)
    assert torch.equal(out.view(torch.int32), ref.view(torch.int32)) and torch.equal(filled, ref_filled)
    import viai_amd
    out2, _, _ = viai_amd.declip(wav, D.CLIP, max_gaps=256, sweeps=2)                           # the package attribute is the same call
    assert torch.equal(out2.view(torch.int32), out.view(torch.int32))


def test_declip_of_a_long_row_equals_the_host_mirrors():
    """257 tiles of `find_gaps`, two per thread of its row launch (declip_common.long_row): clipped runs over a thread edge and up to the last
    sample, which is alone in its tile.  The lists are the host's as integers, `out` and `filled` the host's bit for bit."""
    from viai_amd.declip import declip, declip_fill_host
    from viai_amd.gap_detect import find_gaps_host
    wav = D.long_row()
    out, gaps, filled = declip(torch.from_numpy(wav.copy()).cuda(), D.CLIP, max_gaps=D.LONG_MAX_GAPS)
    want_gaps = find_gaps_host(wav, clip=D.CLIP, min_len=1, max_gaps=D.LONG_MAX_GAPS)
    assert 0 < int(gaps.count[0]) <= D.LONG_MAX_GAPS                                            # the lists hold every run
    assert all(g.dtype == torch.int32 and np.array_equal(g.cpu().numpy(), w) for g, w in zip(gaps, want_gaps))
    want, want_filled = declip_fill_host(wav, want_gaps)
    assert np.array_equal(filled.cpu().numpy(), want_filled) and int((want_filled == 1).sum()) == int(want_gaps.count[0])
    assert np.array_equal(bits(out.cpu().numpy()), bits(want)) and not np.array_equal(bits(want), bits(wav))


@pytest.mark.parametrize("clip", [9830.0 / 32768.0, None])
def test_declip_file_changes_only_the_bytes_of_the_listed_runs(tmp_path, clip):
    import wav_io_common as W
    from viai_amd import wav_io as wio
    from viai_amd.declip import declip_file
    clean, clipped = D.speechlike(3)
    n = clean.size
    if clip is None:                                                                            # driven into the format's full scale
        planes = np.stack([np.clip(3.0 * clean, -1.0, 1.0).astype(np.float32), 0.2 * clean])
    else:
        planes = np.stack([clipped, 0.2 * clean])                                               # channel 1 never reaches the level
    data = W.encode_rule(planes, "s16").tobytes()
    buf = W.wav_file("s16", 2, 16000, data)
    src, dst = str(tmp_path / "src.wav"), str(tmp_path / "dst.wav")
    open(src, "wb").write(buf)
    gaps, info = declip_file(src, dst, clip=clip, max_gaps=512)
    count = gaps.count.tolist()
    assert count[0] >= 40 and max(count) <= 512 and info.channels == 2 and info.frames == n
    out = open(dst, "rb").read()
    off = info.data_offset
    assert len(out) == len(buf) and out[:off] == buf[:off] and out[off + info.data_bytes:] == buf[off + info.data_bytes:]
    old = np.frombuffer(buf, dtype=np.uint8, count=info.data_bytes, offset=off).reshape(n, 2, wio.BYTES["s16"])
    new = np.frombuffer(out, dtype=np.uint8, count=info.data_bytes, offset=off).reshape(n, 2, wio.BYTES["s16"])
    start, length = gaps.start.cpu().numpy(), gaps.length.cpu().numpy()
    inside = np.zeros((n, 2), dtype=bool)
    for ch in range(2):
        for k in range(count[ch]):
            inside[start[ch, k]:start[ch, k] + length[ch, k], ch] = True
    changed = (new != old).any(axis=2)
    assert not changed[~inside].any()
    if clip is not None:
        assert changed[inside[:, 0], 0].mean() > 0.5                                            # the clipped peaks came back above the level
    with pytest.raises(ValueError, match="hold"):
        declip_file(src, str(tmp_path / "never.wav"), clip=clip, max_gaps=2)
