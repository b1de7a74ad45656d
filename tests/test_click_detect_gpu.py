"""GPU: `viai_amd.click_detect.find_clicks` (csrc/click_detect.hip) equals its host mirror as exact integers over the table of
tests/click_detect_common.py (n = 1, 63, 4096, 4097 and 2 * 4096 + 777, ragged lengths, rows that are 4-byte but not 16-byte aligned, order 1
and 128, guard 0 and 64, clicks on both sides of a tile boundary, B = 1 and 5); it repeats, and a row alone is the row in a batch; `declick`
equals `find_clicks_host` + `ar_fill_host` bit for bit and reads the lists where they lie; `declick_file` changes only the bytes of the listed
runs.  The largest clip of the table is 8969 samples; test_device_equals_the_host_mirror_on_a_long_row and
test_declick_of_a_long_row_equals_the_host_mirrors_bit_for_bit run 2 rows of 256 * 4096 + 1 samples (257 tiles: gd_rows_kernel with two tiles per
thread, cd_dilate_kernel and gd_emit_kernel at tile indices far into a row)."""
import numpy as np
import pytest
import torch

import click_detect_common as K

pytestmark = pytest.mark.gpu


def bits(t):
    return t.contiguous().view(torch.int32)


def on_device(c):
    """the clip as a view of its wider rows on the device: what the table's stride says, not a compacted copy"""
    return torch.from_numpy(c["wav"]).cuda()[:, :c["n"]]


_HOST = {}


def host(c):
    from viai_amd.click_detect import find_clicks_host
    if c["name"] not in _HOST:
        _HOST[c["name"]] = find_clicks_host(K.clip(c), **K.call_kwargs(c))
    return _HOST[c["name"]]


def same(got, want):
    assert all(g.is_cuda and g.dtype == torch.int32 for g in got) and tuple(got.start.shape) == want.start.shape
    assert np.array_equal(got.count.cpu().numpy(), want.count), (got.count.tolist(), want.count.tolist())
    assert np.array_equal(got.start.cpu().numpy(), want.start) and np.array_equal(got.length.cpu().numpy(), want.length)


# ----------------------------------------------------------------------------- 1. the device is the host mirror
@pytest.mark.parametrize("name", K.case_names())
def test_device_equals_the_host_mirror_exactly(name):
    from viai_amd.click_detect import find_clicks
    c = K.case_by_name(name)
    wav = on_device(c)
    kept = wav.clone()
    got = find_clicks(wav, **K.call_kwargs(c))
    same(got, host(c))
    assert torch.equal(bits(wav), bits(kept))                             # the input is not written
    again = find_clicks(wav, **K.call_kwargs(c))
    assert all(torch.equal(a, b) for a, b in zip(again, got))


def test_device_equals_the_host_mirror_on_a_long_row():
    """257 tiles, so each thread of gd_rows_kernel owns two and cd_dilate_kernel / gd_emit_kernel index tiles far into the row: clicks whose
    dilation crosses a thread edge, clicks in the last full tile and on the last sample, lengths [n, 255 T + 9]"""
    from viai_amd.click_detect import find_clicks
    c = K.long_case()
    got = find_clicks(on_device(c), **K.call_kwargs(c))
    same(got, host(c))
    assert int(got.count[0]) >= 5 and int(got.count[1]) >= 2              # two thread edges, and in row 0 three clicks in the last full tile


def test_declick_of_a_long_row_equals_the_host_mirrors_bit_for_bit():
    from viai_amd.click_detect import declick, declick_host
    c = K.long_case()
    out, gaps, filled = declick(on_device(c), lengths=c["lengths"])
    want, want_gaps, want_filled = declick_host(K.clip(c), lengths=c["lengths"])
    same(gaps, want_gaps)
    assert np.array_equal(filled.cpu().numpy(), want_filled) and int((filled > 0).sum()) >= 8
    assert np.array_equal(bits(out).cpu().numpy(), np.ascontiguousarray(want).view(np.int32))
    assert not np.array_equal(want.view(np.int32), K.clip(c).view(np.int32))


def test_a_row_view_that_is_not_16_byte_aligned():
    from viai_amd.click_detect import find_clicks
    c = K.case_by_name("base")
    buf = torch.zeros(c["n"] + 8, device="cuda")
    for off in (1, 2, 3):
        buf[off:off + c["n"]] = torch.from_numpy(c["wav"][0]).cuda()
        view = buf[off:off + c["n"]].unsqueeze(0)
        assert view.data_ptr() % 16 != 0 and view.data_ptr() % 4 == 0
        same(find_clicks(view), host(c))


def test_a_row_alone_is_the_row_in_a_batch_of_five():
    from viai_amd.click_detect import find_clicks
    c = K.case_by_name("ragged five")
    wav = on_device(c)
    whole = find_clicks(wav, lengths=c["lengths"])
    assert wav.size(0) == 5
    for b in range(5):
        alone = find_clicks(wav[b:b + 1], lengths=c["lengths"][b:b + 1])
        assert all(torch.equal(a[0], w[b]) for a, w in zip(alone, whole)), b


# ----------------------------------------------------------------------------- 2. declick
def test_declick_equals_the_host_mirrors_bit_for_bit():
    from viai_amd.click_detect import declick, declick_host
    c = K.case_by_name("ragged five")
    wav = on_device(c)
    kept = wav.clone()
    out, gaps, filled = declick(wav, lengths=c["lengths"])
    want, want_gaps, want_filled = declick_host(K.clip(c), lengths=c["lengths"])
    same(gaps, want_gaps)
    assert np.array_equal(filled.cpu().numpy(), want_filled) and int((filled > 0).sum()) == int(np.minimum(want_gaps.count, 64).sum()) > 0
    assert np.array_equal(bits(out).cpu().numpy(), np.ascontiguousarray(want).view(np.int32))
    assert torch.equal(bits(wav), bits(kept)) and out.data_ptr() != wav.data_ptr()
    assert int(gaps.count[1]) == 0 and torch.equal(bits(out[1]), bits(wav[1]))       # a row without clicks keeps its bits
    assert not torch.equal(bits(out[0]), bits(wav[0]))


def test_rows_without_clicks_are_unchanged():
    from viai_amd.click_detect import declick
    clean = torch.from_numpy(np.stack([K.base_signal(s)[0] for s in (0, 1)])).cuda()
    out, gaps, filled = declick(clean)
    assert gaps.count.tolist() == [0, 0] and int(filled.abs().sum()) == 0 and torch.equal(bits(out), bits(clean))


def test_find_clicks_output_is_read_by_ar_fill_where_it_lies(monkeypatch):
    from viai_amd import _lib
    from viai_amd.ar_fill import ar_fill
    from viai_amd.click_detect import find_clicks
    wav = on_device(K.case_by_name("base"))
    gaps = find_clicks(wav)
    ptrs = [g.data_ptr() for g in gaps]
    lib = _lib.load()
    seen = []
    real = lib.viai_ar_fill

    def spy(*args):
        seen.append(args[5:8])
        return real(*args)
    monkeypatch.setattr(lib, "viai_ar_fill", spy)
    out, filled = ar_fill(wav, gaps)
    assert [list(s) for s in seen] == [ptrs] and [g.data_ptr() for g in gaps] == ptrs
    assert int((filled > 0).sum()) == int(gaps.count[0]) == 12


# ----------------------------------------------------------------------------- 3. declick_file
@pytest.mark.parametrize("fmt", ["s16", "f32"])
def test_declick_file_changes_only_the_listed_runs(tmp_path, fmt):
    import wav_io_common as W
    from viai_amd import wav_io as wio
    from viai_amd.click_detect import declick_file
    n = K.TILE + 500
    planes = np.stack([K.clicked(0, n=n, count=4)[1], K.base_signal(1, n=n)[0]])          # channel 1 is clean
    data = W.encode_rule(planes, fmt).tobytes()
    buf = W.wav_file(fmt, 2, 16000, data)
    src, dst = str(tmp_path / "src.wav"), str(tmp_path / "dst.wav")
    open(src, "wb").write(buf)
    gaps, info = declick_file(src, dst)
    assert gaps.count.tolist() == [4, 0] and info.channels == 2 and info.frames == n
    out = open(dst, "rb").read()
    off, fb = info.data_offset, wio.BYTES[fmt]
    assert len(out) == len(buf) and out[:off] == buf[:off] and out[off + info.data_bytes:] == buf[off + info.data_bytes:]
    old = np.frombuffer(buf, dtype=np.uint8, count=info.data_bytes, offset=off).reshape(n, 2, fb)
    new = np.frombuffer(out, dtype=np.uint8, count=info.data_bytes, offset=off).reshape(n, 2, fb)
    inside = np.zeros((n, 2), dtype=bool)
    for k in range(4):
        s, L = int(gaps.start[0, k]), int(gaps.length[0, k])
        inside[s:s + L, 0] = True
    assert np.array_equal(new[~inside], old[~inside])
    changed = (new != old).any(axis=2)
    assert changed[inside].mean() > 0.5 and not changed[~inside].any()
    with pytest.raises(ValueError, match="hold"):
        declick_file(src, str(tmp_path / "never.wav"), max_gaps=2)
    assert not (tmp_path / "never.wav").exists()
