"""No GPU: what the counter-based dropout of the WaveNet residual layers rests on -- a numpy restatement of Philox4x32-10 checked against the
Random123 known-answer vectors, the mask rule restated on it (the GPU test imports both), `viai_dropout` in the built library with its ctypes
signature and host-side refusals, and the Python surface (`dropout`, `dropout_mask`, the seed / state methods of `WaveNet`)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
LO, S32 = np.uint64(0xFFFFFFFF), np.uint64(32)


def philox4x32_10(counter, key):
    """counter: four uint64 arrays (or scalars) holding 32-bit words, key: two Python ints -> the four output words as uint64 arrays"""
    c = [np.asarray(v, dtype=np.uint64) & LO for v in counter]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]                                   # < 2^64: both factors are below 2^32
        c = [(p1 >> S32) ^ c[1] ^ np.uint64(k0), p1 & LO, (p0 >> S32) ^ c[3] ^ np.uint64(k1), p0 & LO]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


def dropout_words(n, seed, offset):
    """word of every element 0 .. n - 1: elements 4 j .. 4 j + 3 are the four outputs of counter (j lo, j hi, offset lo, offset hi), key
    (seed lo, seed hi)"""
    j = np.arange((n + 3) // 4, dtype=np.uint64)
    z = np.zeros_like(j)
    w = philox4x32_10((j & LO, j >> S32, z + np.uint64(offset & 0xFFFFFFFF), z + np.uint64(offset >> 32)), (seed & 0xFFFFFFFF, seed >> 32))
    return np.stack(w, axis=1).reshape(-1)[:n]


def keep_mask(n, p, seed, offset):
    """the keep rule: word >= floor(p * 2^32)"""
    return dropout_words(n, seed, offset) >= np.uint64(int(np.floor(p * 4294967296.0)))


@pytest.fixture(scope="module")
def lib():
    from viai_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_philox_known_answers():
    """the three Random123 known-answer vectors of philox4x32-10"""
    f = 0xFFFFFFFF
    kat = (((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((f, f, f, f), (f, f), "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"))
    for ctr, key, want in kat:
        assert " ".join("%08x" % int(v) for v in philox4x32_10(ctr, key)) == want
    # vectorised over counters: the same words as one call per counter
    many = philox4x32_10((np.array([0, f, 0x243F6A88]), np.array([0, f, 0x85A308D3]), np.array([0, f, 0x13198A2E]), np.array([0, f, 0x03707344])), (0, 0))
    assert " ".join("%08x" % int(v[0]) for v in many) == kat[0][2]


def test_mask_stream_fixed_facts():
    """n = 4096, p = 0.05, seed = 1234, offset = 0 keeps 3912 elements (184 dropped, 0.955078125 of 4096): a fixed fact of the stream the
    GPU test checks the kernel against; the high words of seed and offset, and the offset itself, change the stream"""
    m = keep_mask(4096, 0.05, 1234, 0)
    assert m.dtype == np.bool_ and m.shape == (4096,) and int(m.sum()) == 3912
    assert int(m.sum()) == 0.955078125 * 4096
    assert np.array_equal(keep_mask(4099, 0.05, 1234, 0)[:4096], m)                    # a tail reuses the counter rule
    for seed, offset in ((1234, 1), (1234, 1 << 32), (1234 + (1 << 32), 0), (1235, 0)):
        assert not np.array_equal(keep_mask(4096, 0.05, seed, offset), m), (seed, offset)
    assert keep_mask(4096, 0.0, 1234, 0).all()                                         # thr = 0 keeps every word


def test_library_exports_and_types_viai_dropout(lib):
    from viai_amd import _lib
    assert hasattr(lib, "viai_dropout"), "libviai_hip.so does not export viai_dropout"
    assert "viai_dropout" in _lib.SIGNATURES, "no ctypes signature for viai_dropout"
    res, args = _lib.SIGNATURES["viai_dropout"]
    assert res is C.c_int and args == [C.c_void_p, C.c_void_p, C.c_long, C.c_double, C.c_ulonglong, C.c_ulonglong, C.c_void_p]
    assert lib.viai_dropout.argtypes == args
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "viai_hip.h")).read(), flags=re.S)
    assert re.search(r"int\s+viai_dropout\s*\(\s*const float\*\s*x,\s*float\*\s*y,\s*long\s+n,\s*double\s+p,\s*unsigned long long\s+seed,\s*"
                     r"unsigned long long\s+offset,\s*void\*\s*stream\s*\)\s*;", header)
    assert lib.viai_abi_version() == 20                                                # an additive symbol: the version did not move


def test_host_refusals(lib):
    """refused on the host, before any launch (the pointers are never touched): p < 0, p >= 1, NaN, n < 0; n == 0 is a no-op"""
    for p in (-0.1, 1.0, float("nan"), 1.5, float("inf")):
        assert lib.viai_dropout(0, 0, 16, p, 1, 0, 0) != 0, p
    assert lib.viai_dropout(0, 0, -1, 0.05, 1, 0, 0) != 0
    assert lib.viai_dropout(0, 0, 0, 0.05, 1, 0, 0) == 0
    assert lib.viai_dropout(0, 0, 0, 0.0, (1 << 64) - 1, (1 << 64) - 1, 0) == 0        # the full 64-bit range of seed and offset passes ctypes


def test_python_surface():
    from viai_amd import _lib, wavenet
    for n in ("dropout", "dropout_mask"):
        assert callable(getattr(wavenet, n))
    for n in ("seed_dropout", "dropout_state", "load_dropout_state"):
        assert callable(getattr(wavenet.WaveNet, n))
    x = torch.ones(8)
    for p in (1.5, 1.0, -0.1, float("nan")):
        with pytest.raises(ValueError):
            wavenet.dropout(x, p, 1, 0)
    with pytest.raises(ValueError):
        wavenet.dropout_mask((8,), 1.5, 1, 0)
    with pytest.raises(_lib.ViaiLibraryError):
        wavenet.dropout(x, 0.05, 1, 0)
    assert wavenet.dropout(x, 0.0, 1, 0) is x                                          # p = 0: the tensor itself, no launch, no device needed
    src = open(os.path.join(ROOT, "vision-infused-audio-inpainter-viai_amd", "wavenet.py")).read()
    assert "functional.dropout" not in src


def small_net(dropout=0.05):
    from viai_amd.wavenet import WaveNet
    return WaveNet(out_channels=32, layers=4, stacks=2, residual_channels=16, gate_channels=16, skip_out_channels=8, dropout=dropout,
                   cin_channels=8, upsample_scales=[2, 2])


def test_layer_indices_and_state_round_trip():
    net = small_net()
    assert [f.layer_index for f in net.conv_layers] == [0, 1, 2, 3]
    keys = list(net.state_dict().keys())
    assert all(f._drop_seed is None and f._drop_calls == 0 for f in net.conv_layers)
    assert net.dropout_state() == {"seed": None, "calls": [0, 0, 0, 0]}
    net.seed_dropout(7)
    st = net.dropout_state()
    assert st == {"seed": 7, "calls": [0, 0, 0, 0]}
    net.seed_dropout(2 ** 40 + 3, calls=5)
    assert net.dropout_state() == {"seed": 2 ** 40 + 3, "calls": [5, 5, 5, 5]}
    net.load_dropout_state(st)
    assert net.dropout_state() == st and all(f._drop_seed == 7 and f._drop_calls == 0 for f in net.conv_layers)
    # layers that drew seeds of their own (an unseeded run) round-trip too
    own = {"seed": [3, 4, 5, 6], "calls": [2, 2, 2, 1]}
    net.load_dropout_state(own)
    assert net.dropout_state() == own and [f._drop_seed for f in net.conv_layers] == [3, 4, 5, 6]
    with pytest.raises(ValueError):
        net.load_dropout_state({"seed": 1, "calls": [0, 0]})
    # plain attributes: the checkpoint layout is the reference's
    assert list(net.state_dict().keys()) == keys and not any("drop" in k or "layer_index" in k for k in keys)
    other = small_net(dropout=0.0)
    assert list(other.state_dict().keys()) == keys
