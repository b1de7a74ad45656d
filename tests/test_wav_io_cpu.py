"""CPU: WAV in, WAV out (include/viai_hip.h) without a device.  The numpy statement of the PCM rule on values written out by hand;
the host mirrors (plain C++ from csrc/viai_pcm_rule.h) equal it bit for bit over the table the GPU test runs; which formats round-trip and which
one does not; the reference's save_wav bytes from tests/golden/wav_io.npz; scipy and the stdlib read what write_wav's layout holds; parse_wav;
and every entry point refuses bad arguments before any launch, so also here.  No tolerance anywhere.  Section 2b holds the host mirrors to the
numpy rule on the long clips of the GPU test (2 098 181 frames; a peak behind partial 255; a run of 24 653 samples)."""
import io
import os
import wave

import numpy as np
import pytest
import torch

import wav_io_common as W

ROOT = W.ROOT
INVALID = 1                                                               # hipErrorInvalidValue
f32 = np.float32


@pytest.fixture(scope="module")
def lib():
    from viai_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


@pytest.fixture(scope="module")
def wio(lib):
    from viai_amd import wav_io
    return wav_io


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_tile_constant_is_the_headers(wio):
    assert W.T == wio.TILE and W.T % 16 == 0 and W.T * 64 <= 65536
    assert wio.FORMATS == W.FORMATS and wio.BYTES == W.BYTES
    import viai_amd
    assert viai_amd.repair_file is wio.repair_file and viai_amd.parse_wav is wio.parse_wav and viai_amd.WavInfo is wio.WavInfo


# ----------------------------------------------------------------------------- 1. the numpy rule, on values written out by hand
def le(values, dtype):
    return np.array(values, dtype=dtype).view(np.uint8)


def test_numpy_rule_on_hand_written_values():
    assert W.decode_rule(le([-32768, -1, 0, 32767], "<i2"), "s16", 1).tolist() == [[-1.0, -1 / 32768, 0.0, 32767 / 32768]]
    s24 = np.array([0x00, 0x00, 0x80, 0xFF, 0xFF, 0x7F, 0xFF, 0xFF, 0xFF, 0x01, 0x00, 0x00], dtype=np.uint8)
    assert W.decode_rule(s24, "s24", 1).tolist() == [[-1.0, 8388607 / 8388608, -1 / 8388608, 1 / 8388608]]
    assert W.decode_rule(np.array([0, 128, 255], dtype=np.uint8), "u8", 1).tolist() == [[-1.0, 0.0, 127 / 128]]
    # S32: 2^24 + 1 is a tie and goes to the even 2^24; 2^24 + 3 is a tie and goes up to 2^24 + 4; INT_MAX rounds to 2^31
    got = W.decode_rule(le([(1 << 24) + 1, (1 << 24) + 3, 0x7FFFFFFF, -(1 << 31), -((1 << 24) + 1)], "<i4"), "s32", 1)
    assert got.tolist() == [[2.0 ** -7, ((1 << 24) + 4) / 2.0 ** 31, 1.0, -1.0, -(2.0 ** -7)]]
    assert same_bits(W.decode_rule(le([np.inf, -0.0, np.nan], "<f4"), "f32", 1).view(np.uint32), np.array([[0x7F800000, 0x80000000, 0x7FC00000]], dtype=np.uint32))
    assert W.decode_rule(le([0.1, 1e300, 1e-300], "<f8"), "f64", 1).tolist() == [[float(f32(0.1)), np.inf, 0.0]]
    # interleaving and the downmix: ((x0 + x1) + x2) / 3 in float32
    x = le([1, 2, 4, -32768, -32768, 32767], "<i2")
    assert W.decode_rule(x, "s16", 3).tolist() == [[1 / 32768, -1.0], [2 / 32768, -1.0], [4 / 32768, 32767 / 32768]]
    want = [float(f32(f32(f32(1 / 32768) + f32(2 / 32768)) + f32(4 / 32768)) / f32(3)), float(f32(f32(f32(-1) + f32(-1)) + f32(32767 / 32768)) / f32(3))]
    assert W.decode_rule(x, "s16", 3, mono=True).tolist() == [want]

    enc = lambda vals, fmt: W.encode_rule(np.array([vals], dtype=f32), fmt)
    ulp1 = np.nextafter(f32(1), f32(2))
    assert enc([0.5 / 32768, 1.5 / 32768, 2.5 / 32768, -0.5 / 32768, -1.5 / 32768], "s16").view("<i2").tolist() == [0, 2, 2, 0, -2]     # ties to even
    assert enc([1.0, -1.0, ulp1, np.inf, -np.inf, np.nan, 32766.5 / 32768, 0.99999], "s16").view("<i2").tolist() == [32767, -32768, 32767, 0, 0, 0, 32766, 32767]
    assert enc([1.0, -1.0, ulp1, np.inf, np.nan, 0.0, 0.5 / 128, 1.5 / 128, -127.5 / 128, 126.5 / 128], "u8").tolist() == [255, 0, 255, 128, 128, 128, 128, 130, 0, 254]
    assert enc([1.0, -1.0, ulp1, -np.inf, np.nan, 1 / 8388608], "s24").tolist() == [0xFF, 0xFF, 0x7F, 0, 0, 0x80, 0xFF, 0xFF, 0x7F, 0, 0, 0, 0, 0, 0, 1, 0, 0]
    assert enc([1.0, -1.0, ulp1, 3e38, np.inf, np.nan, 0.5, -2.0 ** -31], "s32").view("<i4").tolist() == [0x7FFFFFFF, -(1 << 31), 0x7FFFFFFF, 0x7FFFFFFF, 0, 0, 1 << 30, -1]
    assert enc([np.inf, np.nan, -0.0], "f32").view("<u4").tolist() == [0x7F800000, 0x7FC00000, 0x80000000]
    assert enc([0.1, -np.inf], "f64").view("<f8").tolist() == [float(f32(0.1)), -np.inf]
    # normalised: the quiet branch, truncation towards zero, non-finite samples outside the peak
    assert W.encode_norm_rule(np.array([[0.005, -0.005, 0.0]], dtype=f32)).view("<i2").tolist() == [int(f32(0.005) * f32(3276700)), -int(f32(0.005) * f32(3276700)), 0]
    p = f32(32767) / f32(65536)
    got = W.encode_norm_rule(np.array([[p, 2.5 / 65536, -2.5 / 65536, (3 - 2.0 ** -8) / 65536, np.inf, np.nan]], dtype=f32)).view("<i2").tolist()
    assert got == [32767, 2, -2, 2, 0, 0]
    assert W.encode_norm_rule(np.array([[0.5], [-1.0]], dtype=f32)).view("<i2").tolist() == [16383, -32767]


# ----------------------------------------------------------------------------- 2. the host mirrors are the numpy rule
@pytest.mark.parametrize("channels", W.CHANNELS)
@pytest.mark.parametrize("fmt", W.FORMATS)
def test_host_mirrors_equal_the_numpy_rule(wio, fmt, channels):
    for frames in W.FRAMES:
        data = W.random_bytes(fmt, channels, frames)
        for mono in (False, True):
            got = wio.decode_pcm_host(data, fmt, channels, mono=mono)
            assert same_bits(got, W.decode_rule(data, fmt, channels, mono)), ("decode", frames, mono)
        wav = W.random_wave(channels, frames)
        assert same_bits(wio.encode_pcm_host(wav, fmt), W.encode_rule(wav, fmt)), ("encode", frames)
        decoded = W.decode_rule(data, fmt, channels)
        with np.errstate(all="ignore"):
            assert same_bits(wio.encode_pcm_host(decoded, fmt), W.encode_rule(decoded, fmt)), ("encode decoded", frames)
        if fmt == "s16":
            assert same_bits(wio.encode_pcm_host(wav, "s16", normalize=True), W.encode_norm_rule(wav)), ("normalised", frames)
            quiet = (wav * f32(0.004)).astype(f32)
            quiet[~np.isfinite(quiet)] = 0
            assert same_bits(wio.encode_pcm_host(quiet, "s16", normalize=True), W.encode_norm_rule(quiet)), ("normalised quiet", frames)
        for variant in (0, 1):
            gaps = W.gaps_case(channels, frames, variant)
            assert same_bits(wio.patch_pcm_host(data, wav, fmt, gaps), W.patch_rule(data, wav, fmt, gaps)), ("patch", frames, variant)


# ----------------------------------------------------------------------------- 2b. the long clips of the GPU test, on the host
def test_long_clips_are_past_the_thresholds_their_names_say():
    tiles = lambda frames: -(-frames // W.T)
    assert tiles(W.LONG_FRAMES) == W.ENCODE_BLOCKS + 2 and W.LONG_FRAMES - (tiles(W.LONG_FRAMES) - 1) * W.T == 5      # block 1's second tile: 5 frames
    assert tiles(W.PEAK_FRAMES) == 300 > W.PEAK_THREADS and all(tile < tiles(frames) for frames, tile in W.PEAK_TILES)
    assert W.LONG_RUN[1] > 3 * W.PATCH_STRIDE and sum(W.LONG_RUN) < W.LONG_FRAMES


@pytest.mark.parametrize("fmt,channels", W.LONG_ENCODE)
def test_host_mirrors_equal_the_numpy_rule_on_a_long_clip(wio, fmt, channels):
    wav = W.random_wave(channels, W.LONG_FRAMES)
    data = wio.encode_pcm_host(wav, fmt)
    assert same_bits(data, W.encode_rule(wav, fmt))
    assert same_bits(wio.decode_pcm_host(data, fmt, channels), W.decode_rule(data, fmt, channels))


@pytest.mark.parametrize("frames,tile", W.PEAK_TILES)
def test_normalised_host_mirror_finds_the_one_peak_of_a_long_clip(wio, frames, tile):
    wav = W.peak_clip(frames, tile)
    got = wio.encode_pcm_host(wav, "s16", normalize=True)
    assert same_bits(got, W.encode_norm_rule(wav))
    assert int(got.view("<i2")[tile * W.T + 1]) <= -32766                # the peak is the planted one (the product is truncated): no inf, no nan


@pytest.mark.parametrize("fmt,channels", W.LONG_PATCH)
def test_patch_host_equals_the_numpy_rule_on_a_long_run(wio, fmt, channels):
    data = W.random_bytes(fmt, channels, W.LONG_FRAMES)
    wav = W.random_wave(channels, W.LONG_FRAMES, seed=5)
    gaps = W.long_patch_gaps(channels)
    assert same_bits(wio.patch_pcm_host(data, wav, fmt, gaps), W.patch_rule(data, wav, fmt, gaps))


# ----------------------------------------------------------------------------- 3. round trips
@pytest.mark.parametrize("fmt", ("u8", "s16", "s24", "f32"))
def test_decode_then_encode_returns_the_bytes(wio, fmt):
    for channels, frames in ((1, W.T + 1), (3, 517), (8, 33)):
        data = W.random_bytes(fmt, channels, frames)
        assert same_bits(wio.encode_pcm_host(wio.decode_pcm_host(data, fmt, channels), fmt), data)


def test_f64_round_trips_when_every_value_is_a_float32(wio):
    x = W.random_wave(2, 300)
    x[~np.isfinite(x)] = 0
    data = np.ascontiguousarray(x.T).astype("<f8").view(np.uint8).reshape(-1)
    assert same_bits(wio.encode_pcm_host(wio.decode_pcm_host(data, "f64", 2), "f64"), data)
    other = le([0.1, 1.0 + 2.0 ** -40], "<f8")                            # not float32 values: the bytes change
    assert not same_bits(wio.encode_pcm_host(wio.decode_pcm_host(other, "f64", 1), "f64"), other)


def test_s32_does_not_round_trip_which_is_why_patch_exists(wio):
    data = le([(1 << 24) + 1, 0x7FFFFFFF, 12345 << 8, -5], "<i4")
    back = wio.encode_pcm_host(wio.decode_pcm_host(data, "s32", 1), "s32")
    assert back.view("<i4").tolist() == [1 << 24, 0x7FFFFFFF, 12345 << 8, -5] and not same_bits(back, data)
    # ... while a patch leaves the samples outside the run alone, bit for bit
    wav = wio.decode_pcm_host(data, "s32", 1)
    gaps = (np.array([1], dtype=np.int32), np.array([[2]], dtype=np.int32), np.array([[1]], dtype=np.int32))
    assert same_bits(wio.patch_pcm_host(data, wav, "s32", gaps), data)


@pytest.mark.parametrize("fmt", W.FORMATS)
def test_patch_host_leaves_every_byte_outside_the_runs(wio, fmt):
    C, n, bps = 3, 2 * W.T + 17, W.BYTES[fmt]
    data = W.random_bytes(fmt, C, n)
    wav = W.random_wave(C, n, seed=1)
    wav[~np.isfinite(wav)] = 0.25
    for variant in (0, 1):
        count, start, length = W.gaps_case(C, n, variant)
        got = wio.patch_pcm_host(data, wav, fmt, (count, start, length)).reshape(n, C, bps)
        inside = np.zeros((n, C), dtype=bool)
        for c in range(C):
            for k in range(min(count[c], 4)):
                inside[max(start[c, k], 0):min(start[c, k] + length[c, k], n), c] = True
        assert inside[0].any() and inside[n - 1].any() and (inside.any(1) & ~inside.all(1)).any()        # a neighbour channel inside a gap's frames
        assert np.array_equal(got[~inside], data.reshape(n, C, bps)[~inside])
        assert np.array_equal(got[inside], W.encode_rule(wav, fmt).reshape(n, C, bps)[inside])
        if count.max() > 4:                                               # the run beyond the lists is not patched: nothing about it is stored
            full = wio.patch_pcm_host(data, wav, fmt, (np.minimum(count, 4), start, length))
            assert same_bits(full.reshape(n, C, bps), got)
    none = (np.zeros(C, dtype=np.int32), np.full((C, 2), 5, dtype=np.int32), np.full((C, 2), 9, dtype=np.int32))
    assert same_bits(wio.patch_pcm_host(data, wav, fmt, none), data)      # count 0: the lists are not looked at


# ----------------------------------------------------------------------------- 4. pins
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "wav_io.npz"))


def test_golden_save_wav_bytes_from_the_host_mirror(wio):
    g = golden()
    rate = int(g["rate"])
    names = [str(n) for n in g["names"]]
    assert len(names) >= 11 and {"tile_minus_1", "tile_plus_1", "peak_f32_0p01", "half_and_almost", "over_32767"} <= set(names)
    assert g["clip.tile_plus_1"].size == W.T + 1 and g["clip.tile_minus_1"].size == W.T - 1
    for name in names:
        clip, want = g["clip." + name], g["file." + name].tobytes()
        data = wio.encode_pcm_host(clip, "s16", normalize=True).tobytes()
        got = wio.wav_header(rate, 1, "s16", clip.size) + data + b"\0" * (len(data) & 1)
        assert got == want, name
        assert W.encode_norm_rule(clip.reshape(1, -1)).tobytes() == data, name


def test_write_layout_is_scipys_and_scipy_reads_every_format(wio):
    wavfile = pytest.importorskip("scipy.io.wavfile")
    rng = np.random.RandomState(5)
    for channels, frames in ((1, 301), (2, 100)):
        q = rng.randint(-32768, 32768, (frames, channels)).astype(np.int16)
        buf = io.BytesIO()
        wavfile.write(buf, 22050, q[:, 0] if channels == 1 else q)
        wav = (q.T.astype(f32) / f32(32768))
        data = wio.encode_pcm_host(wav, "s16").tobytes()
        assert wio.wav_header(22050, channels, "s16", frames) + data == buf.getvalue()
    x = W.random_wave(2, 77)
    x[~np.isfinite(x)] = 0.5
    for fmt in W.FORMATS:
        data = wio.encode_pcm_host(x, fmt).tobytes()
        rate, got = wavfile.read(io.BytesIO(wio.wav_header(8000, 2, fmt, 77) + data + b"\0" * (len(data) & 1)))
        assert rate == 8000 and got.shape == (77, 2)
        raw = np.frombuffer(data, dtype=np.uint8)
        if fmt == "s24":                                                  # scipy hands 24-bit samples back in the high bytes of int32
            want = (W.decode_rule(raw, "s24", 2).T.astype(np.float64) * 2 ** 31).astype(np.int32)
        else:
            want = raw.view({"u8": "u1", "s16": "<i2", "s32": "<i4", "f32": "<f4", "f64": "<f8"}[fmt]).reshape(77, 2)
        assert np.array_equal(got, want), fmt


@pytest.mark.parametrize("fmt", ("u8", "s16", "s24", "s32"))
def test_stdlib_wave_reads_the_integer_files(wio, fmt):
    x = W.random_wave(2, 1001)
    data = wio.encode_pcm_host(x, fmt).tobytes()
    with wave.open(io.BytesIO(wio.wav_header(44100, 2, fmt, 1001) + data + b"\0" * (len(data) & 1)), "rb") as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (2, W.BYTES[fmt], 44100, 1001)
        assert w.readframes(1001) == data


# ----------------------------------------------------------------------------- 5. parsing
def test_parse_wav_layouts(wio, tmp_path):
    data = W.random_bytes("s16", 2, 50).tobytes()
    Info = wio.WavInfo
    plain = W.wav_file("s16", 2, 16000, data)
    assert wio.parse_wav(plain) == Info(16000, 2, "s16", 50, 44, 200)
    p = tmp_path / "a.wav"
    p.write_bytes(plain)
    assert wio.parse_wav(str(p)) == wio.parse_wav(plain) == wio.parse_wav(wio.wav_header(16000, 2, "s16", 50) + data)
    lst = W.chunk(b"LIST", b"INFOISFT\x05\x00\x00\x00abcd\x00\x00")
    assert wio.parse_wav(W.wav_file("s16", 2, 16000, data, extra_before=lst)) == Info(16000, 2, "s16", 50, 44 + len(lst), 200)
    odd = W.chunk(b"junk", b"\x01\x02\x03")                               # 3 bytes and a pad byte
    assert len(odd) == 12
    assert wio.parse_wav(W.wav_file("s16", 2, 16000, data, extra_before=odd + lst)) == Info(16000, 2, "s16", 50, 44 + 12 + len(lst), 200)
    for fmt in W.FORMATS:
        d = W.random_bytes(fmt, 3, 10).tobytes()
        assert wio.parse_wav(W.wav_file(fmt, 3, 48000, d, extensible=True)) == Info(48000, 3, fmt, 10, 44 + 24, len(d))
        assert wio.parse_wav(W.wav_file(fmt, 3, 48000, d)) == Info(48000, 3, fmt, 10, 44, len(d))
        assert wio.parse_wav(wio.wav_header(48000, 3, fmt, 10) + d)[:4] == (48000, 3, fmt, 10)
    after = W.chunk(b"note", b"xy")
    assert wio.parse_wav(W.wav_file("s16", 2, 16000, data, extra_after=after)) == Info(16000, 2, "s16", 50, 44, 200)
    for size in (0, 0xFFFFFFFF, 5000):                                    # "to the end of the file"
        assert wio.parse_wav(W.wav_file("s16", 2, 16000, data, data_size=size)) == Info(16000, 2, "s16", 50, 44, 200)
        assert wio.parse_wav(W.wav_file("s16", 2, 16000, data + b"\x07\x08\x09", data_size=size)) == Info(16000, 2, "s16", 50, 44, 200)
    assert wio.parse_wav(W.wav_file("s16", 2, 16000, data + b"\x07", data_size=201)) == Info(16000, 2, "s16", 50, 44, 200)     # a partial frame
    assert wio.parse_wav(W.wav_file("s24", 3, 16000, b"\0" * 8)) == Info(16000, 3, "s24", 0, 44, 0)


def test_parse_wav_refusals(wio):
    data = b"\0" * 64
    ok = W.wav_file("s16", 2, 16000, data)
    bad = {
        "RF64": b"RF64" + ok[4:],
        "RIFX": b"RIFX" + ok[4:],
        "not a RIFF": b"FORM" + ok[4:],
        "not a RIFF/WAVE": ok[:8] + b"AVI " + ok[12:],
        "bytes are no": ok[:10],
        "tag 0x0002": W.wav_file("s16", 2, 16000, data, tag=2),           # ADPCM
        "tag 0x0007": W.wav_file("u8", 2, 16000, data, tag=7),            # mu-law
        "tag 0x0055": W.wav_file("s16", 2, 16000, data, tag=0x55),        # MP3
        "tag 0x0003 with 16": W.wav_file("s16", 2, 16000, data, tag=3),
        "tag 0x0001 with 64": W.wav_file("f64", 1, 16000, data, tag=1),
        "block_align": ok[:32] + b"\x06\x00" + ok[34:],
        "0 channels": ok[:22] + b"\x00\x00" + ok[24:],
        "9 channels": ok[:22] + b"\x09\x00" + ok[24:],
        "no data chunk": ok[:36],
        "no fmt chunk": ok[:12],
        "before any fmt": ok[:12] + ok[36:] + ok[12:36],
    }
    for what, buf in bad.items():
        with pytest.raises(ValueError, match=what):
            wio.parse_wav(buf)


# ----------------------------------------------------------------------------- 6. refusals, before any launch
def test_every_refusal_is_invalid_value_without_a_device(lib):
    """the pointers of a refused call are never dereferenced: small fake addresses, aligned as the calls want them"""
    src, out, ws, cnt, st, ln = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000

    def decode(host, src=src, fmt=1, channels=2, frames=100, mono=0, out=out, out_stride=100):
        if host:
            return lib.viai_pcm_decode_host(src, fmt, channels, frames, mono, out, out_stride)
        return lib.viai_pcm_decode(src, fmt, channels, frames, mono, out, out_stride, None)

    def encode(host, wav=out, stride=100, channels=2, frames=100, fmt=1, normalize=0, dst=src, ws=ws):
        if host:
            return lib.viai_pcm_encode_host(wav, stride, channels, frames, fmt, normalize, dst)
        return lib.viai_pcm_encode(wav, stride, channels, frames, fmt, normalize, dst, ws, None)

    def patch(host, wav=out, stride=100, channels=2, frames=100, fmt=1, count=cnt, start=st, length=ln, K=4, dst=src):
        if host:
            return lib.viai_pcm_patch_host(wav, stride, channels, frames, fmt, count, start, length, K, dst)
        return lib.viai_pcm_patch(wav, stride, channels, frames, fmt, count, start, length, K, dst, None)

    shape = [dict(fmt=-1), dict(fmt=6), dict(fmt=99), dict(channels=0), dict(channels=9), dict(channels=-1), dict(frames=-1), dict(frames=-(1 << 40))]
    for host in (True, False):
        for kw in shape + [dict(src=None), dict(out=None), dict(out_stride=99)]:
            assert decode(host, **kw) == INVALID, ("decode", host, kw)
        for kw in shape + [dict(wav=None), dict(dst=None), dict(stride=99)] + [dict(normalize=1, fmt=f) for f in (0, 2, 3, 4, 5)]:
            assert encode(host, **kw) == INVALID, ("encode", host, kw)
        for kw in shape + [dict(wav=None), dict(dst=None), dict(count=None), dict(start=None), dict(length=None), dict(stride=99), dict(K=0), dict(K=-3)]:
            assert patch(host, **kw) == INVALID, ("patch", host, kw)
    assert encode(False, normalize=1, ws=None) == INVALID                 # the normalised device call needs its workspace
    assert decode(False, src=0x1004) == INVALID and encode(False, dst=0x1008) == INVALID          # the byte stream is 16-byte aligned
    assert decode(False, out=0x2002) == INVALID and encode(False, wav=0x2001) == INVALID and patch(False, wav=0x2002) == INVALID
    for kw in (dict(wav=None), dict(ws=None), dict(channels=0), dict(channels=9), dict(frames=-1), dict(stride=99)):
        a = dict(wav=out, stride=100, channels=2, frames=100, ws=ws)
        a.update(kw)
        assert lib.viai_pcm_peak(a["wav"], a["stride"], a["channels"], a["frames"], a["ws"], None) == INVALID, kw
    # nothing to do is no error, and launches nothing
    assert decode(False, frames=0, out_stride=0) == 0 and encode(False, frames=0, stride=0) == 0 and patch(False, frames=0, stride=0) == 0
    ws_bytes = lib.viai_pcm_ws_bytes
    assert ws_bytes(-1) == 0 and ws_bytes(0) == 4 and ws_bytes(1) == 4 and ws_bytes(W.T) == 4 and ws_bytes(W.T + 1) == 8 and ws_bytes(1 << 24) == 4 * (1 << 24) // W.T


def test_python_entry_points_check_their_arguments(wio):
    from viai_amd._lib import ViaiLibraryError
    data = torch.zeros(24, dtype=torch.uint8)
    wav = torch.zeros(2, 6)
    gaps = (torch.zeros(2, dtype=torch.int32), torch.zeros(2, 4, dtype=torch.int32), torch.zeros(2, 4, dtype=torch.int32))
    with pytest.raises(ViaiLibraryError):
        wio.decode_pcm(data, "s16", 2)
    with pytest.raises(ViaiLibraryError):
        wio.encode_pcm(wav, "s16")
    with pytest.raises(ViaiLibraryError):
        wio.patch_pcm(data, wav, "s16", gaps)
    for call in (lambda: wio.decode_pcm(data, "s12", 2), lambda: wio.decode_pcm(data, "s16", 9), lambda: wio.decode_pcm(data, "s16", 0),
                 lambda: wio.decode_pcm(data[:23], "s16", 2), lambda: wio.decode_pcm(data.float(), "s16", 2),
                 lambda: wio.encode_pcm(wav, "s24", normalize=True), lambda: wio.encode_pcm(torch.zeros(9, 4), "s16"),
                 lambda: wio.encode_pcm_host(np.zeros((2, 6)), "f32", normalize=True), lambda: wio.decode_pcm_host(np.zeros(23, dtype=np.uint8), "s16", 2),
                 lambda: wio.patch_pcm(data, torch.zeros(2, 5), "s16", gaps), lambda: wio.patch_pcm(data, wav, "s16", gaps[:2] + (gaps[2][:, :3],)),
                 lambda: wio.patch_pcm_host(data.numpy(), np.zeros((2, 6)), "s16", (gaps[0][:1], gaps[1], gaps[2])),
                 lambda: wio.wav_header(16000, 2, "s16", 1 << 31)):
        with pytest.raises(ValueError):
            call()
