"""CPU: the host side of the ragged STFT -> mel call (viai_stft_mel_ragged_plan is host code; viai_stft_mel_ragged refuses bad tables before any
launch; MelFrontEnd.ragged checks its arguments before the library is loaded).  Written against the table layout in include/viai_hip.h."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILY = {1: "r512", 2: "wave", 3: "banded"}               # VIAI_STFT_R512 / _WAVE / _BANDED
TILE = {1: 32, 2: 32, 3: 8}                                # frames per item, as the header states them


@pytest.fixture(scope="module")
def lib():
    from viai_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_symbols_are_declared_exported_and_bound(lib):
    from viai_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "viai_hip.h")).read(), flags=re.S)
    for name in ("viai_stft_mel_ragged_plan", "viai_stft_mel_ragged"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert re.search(r"VIAI_STFT_R512\s*=\s*1,\s*VIAI_STFT_WAVE\s*=\s*2,\s*VIAI_STFT_BANDED\s*=\s*3", text)
    assert lib.viai_abi_version() == _lib.ABI_VERSION == 20


def fixed_rows():
    """lengths 1 .. 70 000 and 300 rows of 512 at offsets that are multiples of 4, odd, and 2 mod 4; rows overlap and leave gaps"""
    lens = [1, 2, 255, 256, 257, 1023, 1024, 8191, 8192, 8193, 70000] + [512] * 300
    offs = [0, 4, 9, 266, 1024, 2049, 4098, 8192, 20001, 30002, 40000] + [120000 + 514 * i + (i % 3) for i in range(300)]
    assert len(lens) == len(offs) == 311
    assert {o % 4 for o in offs} == {0, 1, 2, 3} and any(o % 4 == 2 for o in offs[:11])
    return lens, offs


def ptr(a):
    return None if a is None else a.ctypes.data


def run_plan(lib, lens, offs, hop, n_mels, aligned, fft=1024, cap=None):
    n = len(lens)
    off = np.asarray(offs, dtype=np.int64)
    ln = np.asarray(lens, dtype=np.int32)
    frames, frame_off, fam, per = np.full(n, -7, np.int32), np.full(n + 1, -7, np.int32), np.full(n, -7, np.int32), np.full(3, -7, np.int32)
    need = lib.viai_stft_mel_ragged_plan(ptr(off), ptr(ln), n, fft, hop, n_mels, aligned, ptr(frames), ptr(frame_off), ptr(fam), None, 0, ptr(per))
    if need < 1:
        return need, None
    items = np.full((need if cap is None else cap, 2), -7, np.int32)
    rc = lib.viai_stft_mel_ragged_plan(ptr(off), ptr(ln), n, fft, hop, n_mels, aligned, ptr(frames), ptr(frame_off), ptr(fam), ptr(items), len(items), ptr(per))
    return rc, dict(need=need, frames=frames, frame_off=frame_off, family=fam, items=items, per=per)


def route(lib, n, hop, n_mels, aligned):
    buf = C.create_string_buffer(16)
    assert lib.viai_stft_mel_route(n, 1024, hop, n_mels, int(aligned), buf, 16) == 1
    return buf.value.decode()


@pytest.mark.parametrize("aligned", [1, 0])
@pytest.mark.parametrize("hop", [256, 200, 255])
def test_plan_properties(lib, hop, aligned):
    from viai_amd.audio import lws_num_frames
    lens, offs = fixed_rows()
    rc, p = run_plan(lib, lens, offs, hop, 80, aligned)
    assert rc == 0
    assert p["frames"].tolist() == [lws_num_frames(n, 1024, hop) for n in lens]
    assert p["frame_off"].tolist() == [0] + np.cumsum(p["frames"]).tolist()
    for r, (n, o) in enumerate(zip(lens, offs)):
        row_aligned = (o % 2 == 0) == bool(aligned)            # 4-byte samples: an even offset keeps the base's alignment, an odd one flips it
        assert FAMILY[int(p["family"][r])] == route(lib, n, hop, 80, row_aligned), (r, n, o)
    seen = {FAMILY[int(f)] for f in p["family"]}
    assert seen == ({"banded"} if hop == 255 else {"r512", "wave"})
    # the items: grouped by family in the order r512, wave, banded; every (row, frame) of a family's rows exactly once, tiles from frame 0
    assert int(p["per"].sum()) == p["need"] == len(p["items"]) and (p["per"] >= 0).all()
    at = 0
    for code in (1, 2, 3):
        mine = p["items"][at:at + int(p["per"][code - 1])]
        at += len(mine)
        cover = {}
        for row, f0 in mine.tolist():
            assert 0 <= row < len(lens) and p["family"][row] == code and f0 % TILE[code] == 0 and 0 <= f0 < p["frames"][row]
            cover.setdefault(row, []).append(f0)
        want_rows = [r for r in range(len(lens)) if p["family"][r] == code]
        assert sorted(cover) == want_rows
        for row in want_rows:
            assert cover[row] == list(range(0, int(p["frames"][row]), TILE[code])), row      # in frame order, no tile twice, none missing
    assert len(p["items"]) > 311                                   # the long rows span several tiles


def test_plan_refusals_and_capacity(lib):
    good = ([1024, 600], [0, 1024])
    assert run_plan(lib, *good, 256, 80, 1)[0] == 0
    for lens, offs, kw in (([0, 600], [0, 1024], {}), ([1024, -1], [0, 1024], {}), ([2 ** 29, 600], [0, 1024], {}), ([1024, 600], [0, -4], {}),
                           (*good, dict(fft=512)), (*good, dict(fft=2048)), (*good, dict(hop=0)), (*good, dict(hop=1025)), (*good, dict(n_mels=0))):
        args = dict(hop=256, n_mels=80, fft=1024)
        args.update(kw)
        assert run_plan(lib, lens, offs, args["hop"], args["n_mels"], 1, fft=args["fft"])[0] < 0, (lens, offs, kw)
    one = np.zeros(1, np.int64), np.ones(1, np.int32)
    assert lib.viai_stft_mel_ragged_plan(ptr(one[0]), ptr(one[1]), 0, 1024, 256, 80, 1, None, None, None, None, 0, None) != 0      # n_rows < 1
    assert lib.viai_stft_mel_ragged_plan(None, ptr(one[1]), 1, 1024, 256, 80, 1, None, None, None, None, 0, None) < 0
    # totals past int32: 2^29 - 1 samples a row at hop 1 is 5e8 frames a row
    big = [2 ** 29 - 1] * 5
    assert run_plan(lib, big, [0] * 5, 1, 80, 1)[0] < 0
    # a too-small capacity returns the count and leaves the list alone; the per-row outputs are written all the same
    lens, offs = fixed_rows()
    rc, p = run_plan(lib, lens, offs, 256, 80, 1)
    rc2, q = run_plan(lib, lens, offs, 256, 80, 1, cap=p["need"] - 1)
    assert rc == 0 and rc2 == p["need"] > 0 and (q["items"] == -7).all()
    assert q["frames"].tolist() == p["frames"].tolist() and q["frame_off"].tolist() == p["frame_off"].tolist() and q["per"].tolist() == p["per"].tolist()


def test_launch_refuses_before_any_device_call(lib):
    """null tables, no rows, no items, fft != 1024: non-zero on a machine without a GPU (nothing is launched; the pointers are never read)"""
    t = np.zeros(16, np.int64)
    host = ptr(t)
    per = np.array([1, 0, 0], np.int32)

    def call(wav=host, off=host, ln=host, fr=host, fo=host, items=host, per=per, n_rows=1, fft=1024, hop=256, n_mels=80, out=host):
        return lib.viai_stft_mel_ragged(wav, off, ln, fr, fo, items, ptr(per), n_rows, host, host, host, host, None, out, fft, hop, n_mels, 0, -100.0, 20.0, None)
    for kw in (dict(off=None), dict(ln=None), dict(fr=None), dict(fo=None), dict(items=None), dict(per=None), dict(wav=None), dict(out=None),
               dict(n_rows=0), dict(fft=512), dict(per=np.zeros(3, np.int32)), dict(per=np.array([1, -1, 0], np.int32)),
               dict(hop=255), dict(n_mels=257)):                # the last two: r512 items on a shape the r512 kernel does not take
        assert call(**kw) != 0, kw


def test_ragged_argument_errors_come_before_the_library(monkeypatch):
    from viai_amd import _lib
    from viai_amd.audio import AudioConfig, MelFrontEnd

    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_load)
    front = MelFrontEnd.__new__(MelFrontEnd)                     # no device tensors: the checks need the configuration only
    front.cfg = AudioConfig
    wav = torch.zeros(4096)
    for kw in (dict(lengths=[4000, 97]),                         # a row past the end of wav
               dict(lengths=[1000], offsets=[3097]), dict(lengths=[1000], offsets=[-1]),
               dict(lengths=[1000, 1000], offsets=[0]),         # lengths / offsets mismatch
               dict(lengths=[]), dict(lengths=None),
               dict(lengths=[1000, 0]),                          # length 0
               dict(lengths=[1000], mask=torch.zeros(3))):
        with pytest.raises(ValueError):
            front.ragged(wav, **kw)
    for bad in ([], [torch.zeros(10), torch.zeros(0)], [torch.zeros(2, 5)], torch.zeros(2, 5)):
        with pytest.raises(ValueError):
            front.ragged(bad, lengths=[5] if isinstance(bad, torch.Tensor) else None)
    with pytest.raises(ValueError):
        front.ragged([torch.zeros(10)], lengths=[10])
    # good arguments on the CPU: loud, and still before the library
    with pytest.raises(_lib.ViaiLibraryError):
        front.ragged(wav, lengths=[1000, 3096])
    with pytest.raises(_lib.ViaiLibraryError):
        front.ragged([torch.zeros(100), torch.zeros(7)])
