"""CPU: the host side of the vocoder data preparation (viai_amd.preprocess): chunking, frame layout and the trim rule against the reference's
own results (tests/golden/preprocess.npz, tools/make_preprocess_golden.py), the two new C-ABI symbols and their host refusals, loud failures."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from preprocess_common import chunks_np, start_and_end

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("viai_utt_trim_bounds", "viai_utt_pack")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "preprocess.npz"))


@pytest.fixture(scope="module")
def lib():
    from viai_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_trim_bounds_host_reproduces_the_reference(golden):
    from viai_amd.preprocess import trim_bounds_host
    names, cls, meta = golden["trim.names"], golden["trim.classes"], golden["trim.meta"]
    assert len(names) >= 40 and {"start0", "only01", "last_at_2", "last_at_size_minus_1", "edge_exact_is_silent"} <= set(names.tolist())
    refused = 0
    for name, row, (thr, size, ok, s, e) in zip(names, cls, meta):
        q = row[:size]
        got = trim_bounds_host(q, int(thr))
        assert got == start_and_end(q, int(thr))[:2], name                 # the loops of utils/audio.py:56-67
        if ok:
            assert got == (int(s), int(e)), (name, thr)
        else:                                                              # the reference's asserts fire: the chunk is refused here too
            refused += 1
            assert got[0] == size or got[1] == -1, (name, thr)
        assert trim_bounds_host(torch.as_tensor(q.astype(np.int32)), int(thr)) == got
    assert 0 < refused < len(names)
    # the branches by name, thr = 2
    at = {n: tuple(int(v) for v in m) for n, m in zip(names, meta) if m[0] == 2}
    assert at["start0"][2:] == (1, 0, 5) and at["last_at_2"][2:] == (1, 0, 2) and at["only01"][2] == 0 and at["all_silent"][2] == 0
    assert at["last_at_size_minus_1"][2:] == (1, 3, 7) and at["edge_exact_is_silent"][2:] == (1, 4, 7)


def test_signal_layout_reproduces_the_reference(golden):
    from viai_amd.preprocess import signal_layout
    rows = golden["layout"]
    assert {(1024, 256), (1024, 320)} == {(int(r[0]), int(r[1])) for r in rows}
    rem = set()
    for fft, hop, n, l, r, N in rows.tolist():
        assert signal_layout(n, fft, hop) == (l, r, N, N * hop), (fft, hop, n)
        assert l == fft - hop and n + l + r >= N * hop                      # librivox.py:97
        rem.add(n % hop if n % hop in (0, 1, hop - 1) else -1)
    assert {0, 1} <= rem
    with pytest.raises(ValueError):
        signal_layout(100, 256, 1024)


def test_chunk_bounds_reproduces_the_reference(golden):
    from viai_amd.preprocess import chunk_bounds
    files, length, first = golden["chunks.files"], golden["chunks.length"].tolist(), golden["chunks.first"].tolist()
    chunk = int(files[0][1])
    assert {chunk - 1, chunk, chunk + 1, 3 * chunk + chunk // 2} <= {int(f[0]) for f in files}
    at = 0
    for n, ch, count in files.tolist():
        got = chunk_bounds(n, ch)
        assert got == chunks_np(n, ch) and len(got) == count, n
        assert [b - a for a, b in got] == length[at:at + count] and [a for a, _ in got] == first[at:at + count], n
        at += count
    assert at == len(length)
    assert chunk_bounds(chunk - 1, chunk) == [] and chunk_bounds(chunk, chunk) == [(0, chunk)] and chunk_bounds(chunk + 1, chunk) == [(0, chunk + 1)]
    assert chunk_bounds(3 * chunk + chunk // 2, chunk) == [(0, chunk), (chunk, 2 * chunk), (2 * chunk, 3 * chunk + chunk // 2)]
    with pytest.raises(ValueError):
        chunk_bounds(10, 0)


def test_new_symbols_are_exported_declared_and_bound(lib):
    from viai_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "viai_hip.h")).read(), flags=re.S)
    for n in NEW:
        assert hasattr(lib, n) and n in _lib.SIGNATURES and re.search(r"\b%s\s*\(" % n, text), n
    assert lib.viai_abi_version() == 20 == _lib.ABI_VERSION
    assert "preprocess.hip" in open(os.path.join(ROOT, "vision-infused-audio-inpainter-viai_amd", "csrc", "Makefile")).read()


def test_host_refusals_need_no_device(lib):
    buf = C.create_string_buffer(64)
    p = C.addressof(buf)                                                    # never dereferenced: every call below is refused on the host
    big = 2 ** 31

    def trim(wav=p, n=4096, off=p, ln=p, nc=1, amax=0, rmax=0.999, mu=255, thr=2, sil=127, bounds=p):
        return lib.viai_utt_trim_bounds(wav, n, off, ln, nc, amax, rmax, mu, thr, sil, bounds, 0)

    def pack(wav=p, n=4096, off=p, ln=p, bounds=p, nc=1, max_len=4096, amax=0, rmax=0.999, mode=0, mu=255, fft=1024, hop=256, row_off=p, rows=p,
             rows_cap=4096, sig_off=p, sig=p, sig_cap=8192):
        return lib.viai_utt_pack(wav, n, off, ln, bounds, nc, max_len, amax, rmax, mode, mu, fft, hop, row_off, rows, rows_cap, sig_off, sig, sig_cap, 0)
    for kw in (dict(wav=0), dict(off=0), dict(ln=0), dict(bounds=0), dict(nc=0), dict(nc=-3), dict(n=0), dict(n=big), dict(mu=0), dict(thr=-1)):
        assert trim(**kw) != 0, kw
    for kw in (dict(wav=0), dict(off=0), dict(ln=0), dict(bounds=0), dict(row_off=0), dict(rows=0), dict(sig_off=0), dict(sig=0), dict(nc=0),
               dict(nc=-1), dict(n=0), dict(n=big), dict(hop=1025), dict(hop=0), dict(mode=3), dict(mode=-1), dict(max_len=0), dict(rows_cap=0),
               dict(rows_cap=big), dict(sig_cap=big), dict(mu=0)):
        assert pack(**kw) != 0, kw


def test_bad_arguments_raise_before_the_library_is_loaded(monkeypatch):
    from viai_amd import _lib, preprocess as PP

    def no_load():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", no_load)
    for kw in (dict(input_type="ulaw"), dict(quantize_channels=1), dict(silence_threshold=-1), dict(chunk_samples=0)):
        with pytest.raises(ValueError):
            PP.UtterancePreprocessor(**kw)
    pre = PP.UtterancePreprocessor()
    assert pre.chunk_samples == 128000 and pre.mu == 255 and pre.silence_threshold == 2 and pre.rescaling and pre.rescaling_max == 0.999
    assert not pre.skip_silent and pre.input_type == "mulaw-quantize"
    with pytest.raises(_lib.ViaiLibraryError, match="GPU only; no CPU fallback"):
        pre(torch.zeros(200000))
    with pytest.raises(_lib.ViaiLibraryError, match="GPU only; no CPU fallback"):
        PP.trim_bounds(torch.zeros(4096), [(0, 4096)])
    with pytest.raises(ValueError):
        pre(torch.zeros(2, 4096))


def test_preprocess_is_a_submodule_only():
    import viai_amd
    import viai_amd.preprocess  # noqa: F401
    with pytest.raises(AttributeError):
        viai_amd.UtterancePreprocessor
