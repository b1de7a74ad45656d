"""GPU: `viai_amd.wav_io` (csrc/wav_io.hip) equals its host mirrors BIT FOR BIT -- decode, plain and normalised encode, patch -- over the table of
tests/wav_io_common.py (six formats, 1, 2, 3 and 8 channels, 1 .. 2 T + 17 frames with T = VIAI_PCM_TILE = 1024: a lone frame, the 16-byte edge,
the tile edge, a tail tile), at other storage offsets, with nothing written outside the outputs; the normalised encode gives the reference's
save_wav bytes of tests/golden/wav_io.npz; `patch_pcm` takes `find_gaps`'s tensors as they are; files round-trip; and `repair_file` leaves every
byte outside the detected gaps' samples as it was; `repair(sample_rate=)` and `repair_file` at 11 025 and 44 100 Hz, through `inpaint_at_rate`, are
the composition written out pass by pass, bit for bit.  No tolerance anywhere.  The largest clip of the table is 2 T + 17 = 2065 frames, the
largest of the foreign-rate tests 9000.

Long clips (section 1b, against the numpy rule; tests/test_wav_io_cpu.py holds the host mirrors to the same rule on the same clips):
    test_encode_past_the_capped_grid_equals_the_numpy_rule            2048 T + T + 5 = 2 098 181 frames, 2050 tiles on pcm_encode_kernel's 2048
                                                                      blocks: the `tile += gridDim.x` walk and its trailing barrier
    test_normalised_encode_finds_the_one_peak_of_a_long_clip          300 and 2050 tiles: the `i += PCM_THREADS` loop over the peak partials,
                                                                      the peak behind partial 255
    test_patch_of_a_run_longer_than_the_grid_equals_the_numpy_rule    a run of 3 * 8192 + 77 samples: pcm_patch_kernel's stride of 32 x 256"""
import os
import types

import numpy as np
import pytest
import torch

import wav_io_common as W

pytestmark = pytest.mark.gpu
f32 = np.float32


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_bits(t, a):
    """a device tensor and a numpy array: the same dtype, shape and bytes"""
    g = t.cpu().numpy()
    a = np.ascontiguousarray(a)
    return g.dtype == a.dtype and g.shape == a.shape and g.tobytes() == a.tobytes()


# ----------------------------------------------------------------------------- 1. the table, against the host mirrors
@pytest.mark.parametrize("channels", W.CHANNELS)
@pytest.mark.parametrize("fmt", W.FORMATS)
def test_device_calls_equal_the_host_mirrors(fmt, channels):
    from viai_amd import wav_io as wio
    for frames in W.FRAMES:
        data = W.random_bytes(fmt, channels, frames)
        d = dev(data)
        for mono in (False, True):
            assert same_bits(wio.decode_pcm(d, fmt, channels, mono=mono), wio.decode_pcm_host(data, fmt, channels, mono=mono)), ("decode", frames, mono)
        wav = W.random_wave(channels, frames)
        w = dev(wav)
        assert same_bits(wio.encode_pcm(w, fmt), wio.encode_pcm_host(wav, fmt)), ("encode", frames)
        decoded = wio.decode_pcm_host(data, fmt, channels)                # the formats' whole range, infinities from F64 included
        assert same_bits(wio.encode_pcm(dev(decoded), fmt), wio.encode_pcm_host(decoded, fmt)), ("encode decoded", frames)
        if fmt == "s16":
            assert same_bits(wio.encode_pcm(w, "s16", normalize=True), wio.encode_pcm_host(wav, "s16", normalize=True)), ("normalised", frames)
            quiet = (wav * f32(0.004)).astype(f32)
            quiet[~np.isfinite(quiet)] = 0
            assert same_bits(wio.encode_pcm(dev(quiet), "s16", normalize=True), wio.encode_pcm_host(quiet, "s16", normalize=True)), ("quiet", frames)
        for variant in (0, 1):
            gaps = W.gaps_case(channels, frames, variant)
            got = wio.patch_pcm(d, w, fmt, tuple(dev(g) for g in gaps))
            assert same_bits(got, wio.patch_pcm_host(data, wav, fmt, gaps)), ("patch", frames, variant)
        assert same_bits(d, data) and same_bits(w, wav)                   # inputs are only read


@pytest.mark.parametrize("fmt", ("s16", "s24", "f64"))
def test_storage_offsets_do_not_change_the_result(fmt):
    """the data at a 16-byte aligned offset and at one that is only 4-byte aligned inside a larger tensor; the waveform as a view of wider rows
    whose planes start 4-byte aligned only"""
    from viai_amd import wav_io as wio
    channels, frames = 3, W.T + 17
    data = W.random_bytes(fmt, channels, frames)
    wav = W.random_wave(channels, frames, seed=2)
    want_dec, want_enc = wio.decode_pcm_host(data, fmt, channels), wio.encode_pcm_host(wav, fmt)
    gaps = W.gaps_case(channels, frames)
    want_patch = wio.patch_pcm_host(data, wav, fmt, gaps)
    big = torch.full((data.size + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    wide = torch.full((channels, frames + 7), 9.0, device="cuda")
    wide[:, 3:3 + frames] = dev(wav)
    for off in (16, 4, 1):
        big[off:off + data.size] = dev(data)
        view = big[off:off + data.size]
        assert view.data_ptr() % 16 == off % 16
        assert same_bits(wio.decode_pcm(view, fmt, channels), want_dec), off
        assert same_bits(wio.patch_pcm(view, wide[:, 3:3 + frames], fmt, tuple(dev(g) for g in gaps)), want_patch), off
    assert same_bits(wio.encode_pcm(wide[:, 3:3 + frames], fmt), want_enc)
    assert same_bits(wio.encode_pcm(wide[:, 4:4 + frames], fmt), wio.encode_pcm_host(wide[:, 4:4 + frames].cpu().numpy(), fmt))
    if fmt == "s16":
        assert same_bits(wio.encode_pcm(wide[:, 3:3 + frames], fmt, normalize=True), wio.encode_pcm_host(wav, fmt, normalize=True))
    assert bool((wide[:, :3] == 9.0).all()) and bool((wide[:, 3 + frames:] == 9.0).all())


@pytest.mark.parametrize("fmt,channels", (("u8", 1), ("s24", 3), ("s16", 2), ("f64", 8)))
def test_nothing_is_written_outside_the_outputs(fmt, channels):
    """the C entry points on buffers with guard bytes on both sides, at a tail tile"""
    from viai_amd import _lib
    lib = _lib.load()
    frames, fb = W.T + 5, channels * W.BYTES[fmt]
    f = W.FORMATS.index(fmt)
    data = W.random_bytes(fmt, channels, frames)
    src = dev(data)
    stride = frames + 11                                                  # planes at 4-byte aligned addresses only
    out = torch.full((16 + channels * stride + 16,), -7.0, device="cuda")
    _lib.check(lib.viai_pcm_decode(src.data_ptr(), f, channels, frames, 0, out.data_ptr() + 64, stride, None), "decode")
    torch.cuda.synchronize()
    planes = out[16:16 + channels * stride].reshape(channels, stride)
    assert same_bits(planes[:, :frames].contiguous(), W.decode_rule(data, fmt, channels))
    assert bool((out[:16] == -7.0).all()) and bool((out[16 + channels * stride:] == -7.0).all()) and bool((planes[:, frames:] == -7.0).all())
    dst = torch.full((64 + frames * fb + 64,), 0xCD, dtype=torch.uint8, device="cuda")
    _lib.check(lib.viai_pcm_encode(planes.data_ptr(), stride, channels, frames, f, 0, dst.data_ptr() + 64, None, None), "encode")
    torch.cuda.synchronize()
    with np.errstate(all="ignore"):
        assert same_bits(dst[64:64 + frames * fb], W.encode_rule(W.decode_rule(data, fmt, channels), fmt))
    assert bool((dst[:64] == 0xCD).all()) and bool((dst[64 + frames * fb:] == 0xCD).all())


# ----------------------------------------------------------------------------- 1b. long clips: the capped grid, the peak partials, a strided run
@pytest.mark.parametrize("fmt,channels", W.LONG_ENCODE)
def test_encode_past_the_capped_grid_equals_the_numpy_rule(fmt, channels):
    """2050 tiles on 2048 blocks: blocks 0 and 1 encode a second tile through the same stage, block 1's is the 5-frame tail.  The C entry point
    on a stream with guard bytes on both sides, then the Python call, then the decode of those bytes."""
    from viai_amd import _lib
    from viai_amd import wav_io as wio
    lib = _lib.load()
    frames, fb = W.LONG_FRAMES, channels * W.BYTES[fmt]
    wav = W.random_wave(channels, frames)
    want = W.encode_rule(wav, fmt)
    w = dev(wav)
    dst = torch.full((64 + frames * fb + 64,), 0xCD, dtype=torch.uint8, device="cuda")
    _lib.check(lib.viai_pcm_encode(w.data_ptr(), frames, channels, frames, W.FORMATS.index(fmt), 0, dst.data_ptr() + 64, None, None), "encode")
    torch.cuda.synchronize()
    assert same_bits(dst[64:64 + frames * fb], want)
    assert bool((dst[:64] == 0xCD).all()) and bool((dst[64 + frames * fb:] == 0xCD).all())      # no byte behind the stream is written
    got = wio.encode_pcm(w, fmt)
    assert same_bits(got, want) and same_bits(w, wav)
    assert same_bits(wio.decode_pcm(got, fmt, channels), W.decode_rule(want, fmt, channels))


@pytest.mark.parametrize("frames,tile", W.PEAK_TILES)
def test_normalised_encode_finds_the_one_peak_of_a_long_clip(frames, tile):
    """the peak in a tile whose partial is a thread's first read (0, 255), its second (256), its eighth (2047) and its ninth (2049, the tail)"""
    from viai_amd import wav_io as wio
    wav = W.peak_clip(frames, tile)
    assert same_bits(wio.encode_pcm(dev(wav), "s16", normalize=True), W.encode_norm_rule(wav))


@pytest.mark.parametrize("fmt,channels", W.LONG_PATCH)
def test_patch_of_a_run_longer_than_the_grid_equals_the_numpy_rule(fmt, channels):
    from viai_amd import wav_io as wio
    frames, bps = W.LONG_FRAMES, W.BYTES[fmt]
    data = W.random_bytes(fmt, channels, frames)
    wav = W.random_wave(channels, frames, seed=5)
    gaps = W.long_patch_gaps(channels)
    d = dev(data)
    got = wio.patch_pcm(d, dev(wav), fmt, tuple(dev(g) for g in gaps))
    assert same_bits(got, W.patch_rule(data, wav, fmt, gaps)) and same_bits(d, data)
    inside = np.zeros((frames, channels), dtype=bool)
    for c in range(channels):
        for k in range(int(gaps[0][c])):
            inside[gaps[1][c, k]:gaps[1][c, k] + gaps[2][c, k], c] = True
    assert int(inside.sum()) == W.LONG_RUN[1] + 33
    new = got.cpu().numpy().reshape(frames, channels, bps)
    assert np.array_equal(new[~inside], data.reshape(frames, channels, bps)[~inside])            # every byte outside the runs keeps its value
    assert np.array_equal(new[inside], W.encode_rule(wav, fmt).reshape(frames, channels, bps)[inside])


# ----------------------------------------------------------------------------- 2. the reference's save_wav, on the device
def test_golden_save_wav_bytes_on_the_device(tmp_path):
    from viai_amd import wav_io as wio
    g = np.load(os.path.join(W.ROOT, "tests", "golden", "wav_io.npz"))
    for name in (str(n) for n in g["names"]):
        clip, want = g["clip." + name], g["file." + name].tobytes()
        x = dev(clip)
        before = x.clone()
        path = str(tmp_path / (name + ".wav"))
        wio.save_wav(x, path, sample_rate=int(g["rate"]))
        assert open(path, "rb").read() == want, name
        assert torch.equal(x, before)                                     # unlike the reference, the caller's tensor is not scaled
        again = wio.encode_pcm(x, "s16", normalize=True)
        assert again.cpu().numpy().tobytes() == want[44:44 + 2 * clip.size], name          # two runs, the same bytes


def test_peak_in_another_channel_and_in_the_last_tile():
    from viai_amd import wav_io as wio
    wav = (W.random_wave(2, 2 * W.T + 17, seed=3) * f32(0.25)).astype(f32)
    wav[~np.isfinite(wav)] = 0
    wav[1, 2 * W.T + 16] = -0.9
    assert same_bits(wio.encode_pcm(dev(wav), "s16", normalize=True), W.encode_norm_rule(wav))


# ----------------------------------------------------------------------------- 3. patch_pcm straight from find_gaps
def test_patch_takes_find_gaps_tensors_as_they_are():
    from viai_amd import wav_io as wio
    from viai_amd.gap_detect import find_gaps, find_gaps_host
    C, n = 2, 2 * W.T + 17
    rng = np.random.RandomState(11)
    clean = rng.uniform(0.1, 0.9, (C, n)).astype(f32)
    damaged = clean.copy()
    damaged[0, :70] = 0
    damaged[0, W.T - 40:W.T + 40] = 0
    damaged[1, n - 100:] = 0
    damaged[1, 300:310] = 0                                               # shorter than min_len: no gap
    data = wio.encode_pcm_host(damaged, "s24")
    gaps = find_gaps(dev(damaged), max_gaps=3)
    assert all(t.is_cuda for t in gaps)
    got = wio.patch_pcm(dev(data), dev(clean), "s24", gaps)
    host_gaps = find_gaps_host(damaged, max_gaps=3)
    assert host_gaps.count.tolist() == [2, 1]
    assert same_bits(got, wio.patch_pcm_host(data, clean, "s24", host_gaps))
    want = wio.encode_pcm_host(damaged, "s24").reshape(n, C, 3)
    full = wio.encode_pcm_host(clean, "s24").reshape(n, C, 3)
    want[:70, 0], want[W.T - 40:W.T + 40, 0], want[n - 100:, 1] = full[:70, 0], full[W.T - 40:W.T + 40, 0], full[n - 100:, 1]
    assert same_bits(got, want.reshape(-1))


# ----------------------------------------------------------------------------- 4. files
@pytest.mark.parametrize("fmt", W.FORMATS)
def test_write_then_read_round_trips(fmt, tmp_path):
    from viai_amd import wav_io as wio
    wav = W.random_wave(2, W.T + 3, seed=4)
    wav[~np.isfinite(wav)] = -0.5
    path = str(tmp_path / "x.wav")
    wio.write_wav(path, dev(wav), 22050, fmt)
    got, info = wio.read_wav(path)
    data = wio.encode_pcm_host(wav, fmt)
    assert info[:4] == (22050, 2, fmt, W.T + 3) and info.data_bytes == data.size
    assert got.is_cuda and same_bits(got, wio.decode_pcm_host(data, fmt, 2))
    mono, _ = wio.read_wav(path, mono=True)
    assert same_bits(mono, wio.decode_pcm_host(data, fmt, 2, mono=True))
    if fmt in ("f32", "f64"):
        assert same_bits(got, wav)
    if fmt != "s32":                                                      # what was read, written again: the same file (S32 does not round-trip)
        first = open(path, "rb").read()
        wio.write_wav(path, got, 22050, fmt)
        assert open(path, "rb").read() == first


RATE, HOP = 16000, 256


def ramp(row, i):
    """what the stub inpainter writes at sample i of row `row`: multiples of 2^-10, exact in every format"""
    return ((i % 200) - 100).to(torch.float32) / 256 + row / 1024


class StubInpainter:
    """called like an AudioInpainter; writes `ramp` into the gaps it is handed and notes what it saw"""
    front = types.SimpleNamespace(cfg=types.SimpleNamespace(sample_rate=RATE, hop_size=HOP))

    def __init__(self):
        self.calls = []

    def __call__(self, wav, gap_start, gap_len, video=None, flow=None, uniforms=None, fade=0, return_parts=False):
        starts, lens = [int(v) for v in gap_start], [int(v) for v in gap_len]
        self.calls.append((tuple(wav.shape), starts, lens))
        out = wav.float().clone()
        for b, (s, l) in enumerate(zip(starts, lens)):
            if l > 0:
                out[b, s:s + l] = ramp(b, torch.arange(s, s + l, device=wav.device))
        return out


def damaged_file(fmt, channels, n, gaps, rate=RATE, tail=b""):
    """(file bytes, data bytes): nonzero samples with exact zeros in the gaps, a LIST chunk in front of the data and a chunk behind it; `tail`:
    the bytes of a partial frame at the end of the data chunk"""
    rng = np.random.RandomState(n + channels)
    wav = (rng.randint(100, 30000, (channels, n)) * rng.choice([-1, 1], (channels, n))).astype(f32) / f32(32768)
    for c, runs in enumerate(gaps):
        for s, e in runs:
            wav[c, s:e] = 0
    data = W.encode_rule(wav, fmt).tobytes()
    before, after = W.chunk(b"LIST", b"INFOISFT\x03\x00\x00\x00abc\x00"), W.chunk(b"note", b"kept")
    return W.wav_file(fmt, channels, rate, data + tail, extra_before=before, extra_after=after), data


@pytest.mark.parametrize("fmt,channels", (("s16", 2), ("s24", 1)))
def test_repair_file_keeps_every_byte_outside_the_gaps(fmt, channels, tmp_path):
    from viai_amd import wav_io as wio
    from viai_amd.gap_detect import find_gaps_host
    n = 5 * HOP + 77
    gaps = [[(300, 400), (n - 150, n)], [(500, 620), (n - 90, n)]][:channels]
    buf, data = damaged_file(fmt, channels, n, gaps)
    src, dst = str(tmp_path / "src.wav"), str(tmp_path / "dst.wav")
    open(src, "wb").write(buf)
    stub = StubInpainter()
    got_gaps, info = wio.repair_file(stub, src, dst)
    assert info == wio.parse_wav(buf) and info[:4] == (RATE, channels, fmt, n)
    decoded = wio.decode_pcm_host(np.frombuffer(data, dtype=np.uint8), fmt, channels)
    want_gaps = find_gaps_host(decoded)
    for g, w in zip(got_gaps, want_gaps):
        assert g.is_cuda and np.array_equal(g.cpu().numpy(), w)
    assert want_gaps.count.tolist() == [2] * channels
    assert [list(map(int, want_gaps.start[c, :2])) for c in range(channels)] == [[s for s, _ in r] for r in gaps]
    # the stub: two passes on whole hops, and no gap reaches into the zero padding
    assert len(stub.calls) == 2
    for shape, starts, lens in stub.calls:
        assert shape == (channels, 6 * HOP)
        assert all(s + l <= n for s, l in zip(starts, lens))
    assert [c[1] for c in stub.calls] == [[r[k][0] for r in gaps] for k in range(2)]
    out = open(dst, "rb").read()
    assert len(out) == len(buf)
    bps, off = W.BYTES[fmt], info.data_offset
    assert out[:off] == buf[:off] and out[off + info.data_bytes:] == buf[off + info.data_bytes:]          # header and chunks
    got = np.frombuffer(out, dtype=np.uint8, count=info.data_bytes, offset=off).reshape(n, channels, bps)
    old = np.frombuffer(data, dtype=np.uint8).reshape(n, channels, bps)
    inside = np.zeros((n, channels), dtype=bool)
    want = np.zeros((channels, n), dtype=f32)
    for c, runs in enumerate(gaps):
        for s, e in runs:
            inside[s:e, c] = True
            want[c, s:e] = ramp(c, torch.arange(s, e)).numpy()
    assert np.array_equal(got[~inside], old[~inside])                     # the other channel's samples inside a gap's frames included
    assert np.array_equal(got[inside], W.encode_rule(want, fmt).reshape(n, channels, bps)[inside])
    assert inside[n - 1].any() and (got[inside] != old[inside]).any()


def test_repair_file_refuses_three_channels_and_an_overflow_before_writing(tmp_path):
    from viai_amd import wav_io as wio
    n = 3 * HOP + 5
    buf, _ = damaged_file("s16", 3, n, [[(100, 200)], [], []])
    src, dst = str(tmp_path / "src.wav"), str(tmp_path / "dst.wav")
    open(src, "wb").write(buf)
    stub = StubInpainter()
    with pytest.raises(ValueError, match="3 channels"):
        wio.repair_file(stub, src, dst)
    assert stub.calls == [] and not os.path.exists(dst)
    buf, _ = damaged_file("s16", 2, n, [[(100, 200), (300, 400), (500, 600)], []])
    open(src, "wb").write(buf)
    with pytest.raises(ValueError, match="hold"):
        wio.repair_file(stub, src, dst, max_gaps=2)                       # three gaps, lists of two: never half repaired
    assert stub.calls == [] and not os.path.exists(dst)


def test_repair_at_the_front_ends_rate_is_the_direct_call():
    """repair(sample_rate=the front end's) calls the inpainter exactly as repair() without the argument does"""
    from viai_amd.gap_detect import repair
    wav = torch.rand(2, 4 * HOP, device="cuda") * 0.8 + 0.1
    wav[0, 100:200] = 0
    wav[1, 700:] = 0
    a, b = StubInpainter(), StubInpainter()
    out_a, gaps_a = repair(a, wav)
    out_b, gaps_b = repair(b, wav, sample_rate=RATE)
    assert a.calls == b.calls and len(a.calls) == 1 and torch.equal(out_a, out_b)
    assert all(torch.equal(x, y) for x, y in zip(gaps_a, gaps_b))


# ----------------------------------------------------------------------------- 5. files and clips at another rate than the front end's
# 11 025 Hz: the down leg (11 025 -> 16 000, L = 640) takes the resampler's consecutive form and the up leg (L = 441) its period form;
# 44 100 Hz: the period form both ways.  n is chosen so that the low-rate clip is no whole number of hops.
FOREIGN = {11025: 4000, 44100: 9000}


def bits(t):
    return t.contiguous().view(torch.int32)


def runs_of(n, channels=2):
    """row 0 holds three runs, the last one up to the clip's end; row 1 holds one, so its later passes see length 0"""
    return [[(300, 400), (1500, 1570), (n - 150, n)], [(700, 820)]][:channels]


def composition(wav, rate, count, start, length):
    """`repair(stub, wav, gaps=, sample_rate=rate)` written out from the public pieces, pass by pass: down to whole hops, the gap widened, the
    stub, up over the run only into a clone.  Returns (the result after every pass, the stub's calls)."""
    from viai_amd.wav_resample import Resampler, gap_at_rate
    down, up = Resampler(rate, RATE), Resampler(RATE, rate)
    stub = StubInpainter()
    n = wav.size(1)
    m = -(-down.out_len(n) // HOP) * HOP
    assert down.out_len(n) % HOP != 0
    steps = [wav.float().clone()]
    for k in range(int(max(count))):
        gs = [int(start[b][k]) if k < int(count[b]) else 0 for b in range(len(count))]
        gl = [int(length[b][k]) if k < int(count[b]) else 0 for b in range(len(count))]
        low = down(steps[-1], out_len=m)
        low_start, low_len = gap_at_rate(gs, gl, down, m)
        low_out = stub(low, low_start, low_len)
        nxt = steps[-1].clone()
        up(low_out, out=nxt, window=(gs, [s + l for s, l in zip(gs, gl)]), out_len=n)
        steps.append(nxt)
    return steps[1:], stub.calls


@pytest.mark.parametrize("rate", sorted(FOREIGN))
def test_repair_at_another_rate_is_the_composition_pass_by_pass(rate):
    from viai_amd.gap_detect import Gaps, repair
    from viai_amd.wav_resample import Resampler
    n, K = FOREIGN[rate], 4
    assert Resampler(rate, RATE).launch_form()[0] == (1 if rate == 11025 else 4) and Resampler(RATE, rate).launch_form()[0] == 4
    runs = runs_of(n)
    wav = torch.rand(2, n, generator=torch.Generator().manual_seed(rate)) * 0.8 + 0.1
    count = torch.tensor([len(r) for r in runs], dtype=torch.int32)
    start, length = torch.zeros(2, K, dtype=torch.int32), torch.zeros(2, K, dtype=torch.int32)
    inside = torch.zeros(2, n, dtype=torch.bool)
    for b, row in enumerate(runs):
        for k, (s, e) in enumerate(row):
            wav[b, s:e] = 0
            start[b, k], length[b, k] = s, e - s
            inside[b, s:e] = True
    wav, inside = wav.cuda(), inside.cuda()
    before = wav.clone()
    stub = StubInpainter()
    out, gaps = repair(stub, wav, gaps=Gaps(count.cuda(), start.cuda(), length.cuda()), sample_rate=rate)
    steps, calls = composition(wav, rate, count, start, length)
    m = -(-Resampler(rate, RATE).out_len(n) // HOP) * HOP
    assert tuple(out.shape) == (2, n) and torch.equal(bits(wav), bits(before))
    assert len(stub.calls) == 3 and stub.calls == calls and all(c[0] == (2, m) for c in calls)
    assert [c[2][1] for c in calls][1:] == [0, 0] and all(c[2][0] > 0 for c in calls) and calls[0][2][1] > 0
    assert torch.equal(bits(out), bits(steps[-1]))                        # bit for bit the composition
    assert torch.equal(bits(out)[~inside], bits(wav)[~inside])            # every sample outside the listed runs keeps the input's bits
    for b, row in enumerate(runs):
        for s, e in row:
            assert int((out[b, s:e] != 0).sum()) > (e - s) // 2, (b, s)   # and the runs were written
    # a pass with length 0 changes nothing in its row: row 1 after passes 2 and 3 is row 1 after pass 1, in the composition and in repair()
    assert torch.equal(bits(steps[1][1]), bits(steps[0][1])) and torch.equal(bits(steps[2][1]), bits(steps[0][1]))
    one, _ = repair(StubInpainter(), wav, gaps=Gaps(count.clamp(max=1), start[:, :1], length[:, :1]), sample_rate=rate)
    assert torch.equal(bits(one), bits(steps[0])) and torch.equal(bits(one[1]), bits(out[1]))


@pytest.mark.parametrize("fmt,channels,rate", (("s16", 2, 11025), ("s24", 1, 11025), ("s16", 2, 44100)))
def test_repair_file_at_another_rate_is_the_composition_and_keeps_every_other_byte(fmt, channels, rate, tmp_path):
    from viai_amd import wav_io as wio
    from viai_amd.gap_detect import find_gaps_host
    n = FOREIGN[rate]
    runs = runs_of(n, channels)
    tail = b"\x07\x08"                                                    # a partial frame behind the last whole one
    buf, data = damaged_file(fmt, channels, n, runs, rate=rate, tail=tail)
    src, dst = str(tmp_path / "src.wav"), str(tmp_path / "dst.wav")
    open(src, "wb").write(buf)
    stub = StubInpainter()
    got_gaps, info = wio.repair_file(stub, src, dst)
    bps, off = W.BYTES[fmt], info.data_offset
    assert info == wio.parse_wav(buf) and info[:4] == (rate, channels, fmt, n) and info.data_bytes == n * channels * bps == len(data)
    # detection ran on the clip at its own length and rate: the runs as they lie in the file, the last one ending at sample n, nothing beyond
    decoded = wio.decode_pcm_host(np.frombuffer(data, dtype=np.uint8), fmt, channels)
    want_gaps = find_gaps_host(decoded)
    for g, w in zip(got_gaps, want_gaps):
        assert g.is_cuda and np.array_equal(g.cpu().numpy(), w)
    assert want_gaps.count.tolist() == [len(r) for r in runs]
    for c, row in enumerate(runs):
        assert [(int(want_gaps.start[c, k]), int(want_gaps.start[c, k] + want_gaps.length[c, k])) for k in range(len(row))] == row
    assert int((want_gaps.start + want_gaps.length).max()) == n
    # the composition on the decoded clip: the same calls of the stub, on whole hops of the front end's grid
    steps, calls = composition(dev(decoded), rate, want_gaps.count, want_gaps.start, want_gaps.length)
    assert stub.calls == calls and len(calls) == max(len(r) for r in runs)
    assert all(c[0][0] == channels and c[0][1] % HOP == 0 for c in calls)
    out = open(dst, "rb").read()
    assert len(out) == len(buf)
    end = off + info.data_bytes
    assert out[:off] == buf[:off] and out[end:] == buf[end:]              # header, the LIST chunk, the partial frame and the chunk behind it
    assert buf[end:end + len(tail)] == tail and b"note" in buf[end:] and b"LIST" in buf[:off]
    got = np.frombuffer(out, dtype=np.uint8, count=info.data_bytes, offset=off).reshape(n, channels, bps)
    old = np.frombuffer(data, dtype=np.uint8).reshape(n, channels, bps)
    inside = np.zeros((n, channels), dtype=bool)
    for c, row in enumerate(runs):
        for s, e in row:
            inside[s:e, c] = True
    assert np.array_equal(got[~inside], old[~inside])                     # every byte outside the detected runs' samples
    want = wio.encode_pcm_host(steps[-1].cpu().numpy(), fmt).reshape(n, channels, bps)
    assert np.array_equal(got[inside], want[inside])
    assert inside[n - 1].any() and (got[inside] != old[inside]).any()
