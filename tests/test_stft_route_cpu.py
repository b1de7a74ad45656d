"""CPU: the route table of the STFT -> mel front end (viai_stft_mel_route: host code, nothing is launched).  viai_stft_mel_banded launches by the
same decision function, so what is pinned here is what tests/test_stft_mel_routes_gpu.py reaches by shape."""
import ctypes as C
import os

import pytest


@pytest.fixture(scope="module")
def lib():
    from viai_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def family(lib, n, fft, hop, n_mels, aligned, cap=16):
    buf = C.create_string_buffer(b"?" * 15, 16)
    ok = lib.viai_stft_mel_route(n, fft, hop, n_mels, aligned, buf, cap)
    assert ok in (0, 1) and (ok == 1) == (buf.value != b"")
    return buf.value.decode()


def test_product_shape_and_each_way_off_it(lib):
    n = 65536
    assert family(lib, n, 1024, 256, 80, 1) == "r512"                    # the product: AudioInpainter's clips, 80 mels, torch allocations
    assert family(lib, n, 1024, 256, 256, 1) == "r512"
    # each of the two conditions alone
    assert family(lib, n + 1, 1024, 256, 80, 1) == "wave"                # an odd clip length: clip 1 starts off an 8-byte boundary
    assert family(lib, n, 1024, 256, 80, 0) == "wave"                    # the first clip itself does
    assert family(lib, n, 1024, 200, 80, 0) == "wave" and family(lib, n + 1, 1024, 1024, 80, 1) == "wave"
    # a hop that is no multiple of 8 leaves both wave kernels: their zero padding left of the clip was measured wrong there (csrc/audio.hip, stft_route)
    for hop in (255, 254, 257, 252, 4, 1):
        assert family(lib, n, 1024, hop, 80, 1) == "banded" and family(lib, n + 1, 1024, hop, 513, 0) == "banded", hop
    # the shapes of tests/test_audio_gpu.py: 5001 samples reach the wave kernel, the other three r512
    assert [family(lib, s, 1024, 256, m, 1) for m, s in ((80, 16384), (256, 65536), (80, 5000), (80, 5001))] == ["r512", "r512", "r512", "wave"]


def test_band_count_thresholds(lib):
    for n_mels, want in ((1, "r512"), (256, "r512"), (257, "wave"), (513, "wave"), (1024, "wave"), (1025, "banded"), (4096, "banded")):
        assert family(lib, 5120, 1024, 256, n_mels, 1) == want, n_mels
    for n_mels, want in ((256, "wave"), (1024, "wave"), (1025, "banded")):
        assert family(lib, 5121, 1024, 256, n_mels, 1) == want, n_mels       # nothing but the band count keeps a shape off the banded kernel
    assert family(lib, 5120, 1024, 1024, 80, 1) == "r512" and family(lib, 5120, 1024, 8, 80, 1) == "r512" and family(lib, 5121, 1024, 8, 80, 1) == "wave"


def test_other_fft_sizes_are_the_dense_kernel_or_refused(lib):
    assert family(lib, 5120, 512, 128, 300, 1) == "dense" and family(lib, 5121, 2048, 511, 1025, 0) == "dense"
    for bad in ((5120, 256, 64, 80), (5120, 1000, 250, 80), (5120, 4096, 1024, 80),      # fft sizes no entry point serves
                (5120, 1024, 0, 80), (5120, 1024, 1025, 80), (5120, 512, 513, 80),      # hop outside 1 .. fft
                (5120, 1024, 256, 0)):
        assert family(lib, bad[0], bad[1], bad[2], bad[3], 1) == "", bad


def test_name_is_truncated_to_the_buffer(lib):
    buf = C.create_string_buffer(b"??????", 7)
    assert lib.viai_stft_mel_route(5120, 1024, 256, 1025, 1, buf, 4) == 1 and buf.raw == b"ban\0??\0"
    assert lib.viai_stft_mel_route(5120, 1024, 256, 1025, 1, None, 0) == 1
