"""Waveform in, waveform out (`viai_amd.inpaint`), the parts that need no GPU: `gap_frames` against the definition it abbreviates, the frame
grid of the mel front end against the vocoder's, the refusals of `AudioInpainter` and of `inpaint_waveform(..., gap_unit=)`, the new C symbols."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

NEW = ("viai_gap_frame_mask", "viai_wav_align", "viai_mel_compose")


def brute(a0, a1, fft, hop, frames):
    """the definition: the frames whose window [j hop, j hop + fft) shares a sample with [a0, a1)"""
    hit = [j for j in range(frames) if any(a0 <= s < a1 for s in range(j * hop, j * hop + fft))]
    if not hit:
        return (0, 0)
    assert hit == list(range(hit[0], hit[-1] + 1))
    return (hit[0], len(hit))


def brute_all(a0, a1, fft, hop, frames):
    """the same definition for many gaps at once: a loop over the frames, each testing whether the two intervals intersect"""
    a0, a1 = np.asarray(a0, dtype=np.int64), np.asarray(a1, dtype=np.int64)
    hit = np.stack([np.maximum(a0, j * hop) < np.minimum(a1, j * hop + fft) for j in range(frames)], 1)
    count = hit.sum(1)
    first = np.where(count > 0, hit.argmax(1), 0)
    assert (hit == ((np.arange(frames)[None] >= first[:, None]) & (np.arange(frames)[None] < (first + count)[:, None]))).all()   # one run of frames
    return first.tolist(), count.tolist()


@pytest.mark.parametrize("fft,hop", [(1024, 256), (8, 3), (4, 4)])
def test_gap_frames_is_the_interval_intersection_exhaustively(fft, hop):
    from viai_amd import gap_frames
    frames = 12
    end = frames * hop
    a0, a1 = np.triu_indices(end + 1)                                    # every 0 <= a0 <= a1 <= frames * hop
    assert len(a0) == (end + 1) * (end + 2) // 2
    want = brute_all(a0, a1, fft, hop, frames)
    if fft <= 8:                                                         # where the sample-by-sample form is affordable, it agrees
        for x, y, f, c in zip(a0.tolist(), a1.tolist(), *want):
            assert brute(x, y, fft, hop, frames) == (f, c), (x, y)
    first, count = gap_frames(torch.from_numpy(a0), torch.from_numpy(a1), fft, hop, frames)      # one entry per stream
    bad = [k for k in range(len(a0)) if (first[k], count[k]) != (want[0][k], want[1][k])][:5] if (first, count) != want else []
    assert not bad, [(int(a0[k]), int(a1[k]), first[k], count[k], want[0][k], want[1][k]) for k in bad]
    k = int(np.flatnonzero((a0 == 5) & (a1 == 7))[0])
    assert gap_frames(5, 7, fft, hop, frames) == (want[0][k], want[1][k])                        # ints in, ints out
    assert gap_frames([5, 0], [7, 0], fft, hop, frames) == ([want[0][k], 0], [want[1][k], 0])    # sequences in, lists out


def test_a_frame_aligned_gap_is_three_frames_wider_on_the_left():
    from viai_amd import gap_frames
    fft, hop, frames = 1024, 256, 208
    for f0 in range(0, 60):
        for L in (1, 2, 13, 52):
            first, count = gap_frames(f0 * hop, (f0 + L) * hop, fft, hop, frames)
            lo = max(f0 - 3, 0)
            assert (first, count) == (lo, f0 + L - lo), (f0, L)
    assert gap_frames(205 * hop, 208 * hop, fft, hop, frames) == (202, 6)
    assert gap_frames(100, 100, fft, hop, frames) == (0, 0)              # an empty gap damages nothing


def test_front_end_frames_times_hop_is_the_aligned_length():
    from viai_amd.audio import AudioConfig, MelFrontEnd, lws_num_frames, lws_pad_lr
    front = MelFrontEnd(AudioConfig, device="cpu")
    fft, hop = AudioConfig.fft_size, AudioConfig.hop_size
    for k in list(range(1, 40)) + [205, 1000]:
        n = k * hop
        frames = front.num_frames(n)
        assert frames == k + 3 and frames * hop == n + (fft - hop)
        l, r = lws_pad_lr(n, fft, hop)                                   # utils/librivox.py:92-102 pads with these and cuts to frames * hop
        assert l == fft - hop and n + l + r >= frames * hop
    for fsize, fshift in ((8, 2), (16, 4), (12, 4)):                     # the identity is lws's, for any fft a multiple of the hop
        for k in range(1, 9):
            assert lws_num_frames(k * fshift, fsize, fshift) * fshift == k * fshift + (fsize - fshift)


def make_vocoder(scales=(4, 4, 4, 4), cin=80, onehot=False):
    from viai_amd.wavenet import WaveNet
    torch.manual_seed(5)
    return WaveNet(out_channels=8 if onehot else 30, layers=4, stacks=2, residual_channels=8, gate_channels=8, skip_out_channels=8, cin_channels=cin,
                   upsample_scales=scales, scalar_input=not onehot, weight_normalization=False).eval()


def make_inpainter(use_video=False):
    """the checks in front of the device need the front end's grid and the vocoder's; the generator is not reached"""
    from viai_amd import AudioInpainter
    from viai_amd.audio import AudioConfig, MelFrontEnd
    model = types.SimpleNamespace(train=1, use_video=use_video, device=torch.device("cpu"))
    return AudioInpainter(model, make_vocoder(), MelFrontEnd(AudioConfig, device="cpu")), model


def test_the_constructor_refuses_a_vocoder_on_another_grid():
    from viai_amd import AudioInpainter
    from viai_amd.audio import AudioConfig, MelFrontEnd
    front = MelFrontEnd(AudioConfig, device="cpu")
    model = types.SimpleNamespace(train=1, use_video=False, device=torch.device("cpu"))
    with pytest.raises(ValueError, match="hops 256"):
        AudioInpainter(model, make_vocoder(scales=(4, 4, 4)), front)
    with pytest.raises(ValueError, match="80 mel bands"):
        AudioInpainter(model, make_vocoder(cin=64), front)
    assert AudioInpainter(model, make_vocoder(), front).front is front


def test_the_call_refuses_bad_arguments_before_the_device():
    inp, model = make_inpainter()
    hop = 256
    wav = torch.zeros(2, 8 * hop)
    with pytest.raises(ValueError, match="whole number"):
        inp(torch.zeros(2, 8 * hop + 1), 100, 10)
    with pytest.raises(ValueError, match=r"\(B, n\)"):
        inp(torch.zeros(8 * hop), 100, 10)
    for start, length in ((-1, 10), (100, -1), (8 * hop - 5, 6), ([0, 8 * hop], [1, 1])):
        with pytest.raises(ValueError, match="inside the clip"):
            inp(wav, start, length)
    with pytest.raises(ValueError, match="per stream"):
        inp(wav, [1, 2, 3], [1, 1, 1])
    for B in (3, 5, 16):
        with pytest.raises(ValueError, match="1, 2, 4 or 8"):
            inp(torch.zeros(B, 8 * hop), 100, 10)
    with pytest.raises(ValueError, match="fade"):
        inp(wav, 100, 10, fade=-1)
    # the generator's width rule bites with the visual branch: 11 frames -> a bottleneck 1 step wide, 8 video frames -> 2
    inp_v, _ = make_inpainter(use_video=True)
    with pytest.raises(ValueError, match="bottleneck"):
        inp_v(wav, 100, 10, video=torch.zeros(2, 8, 3, 2, 2), flow=torch.zeros(2, 8, 2, 2, 2))
    # arguments that pass reach the device check (and nothing was changed on the way)
    from viai_amd._lib import ViaiLibraryError
    with pytest.raises(ViaiLibraryError, match="GPU only"):
        inp(wav, [0, 8 * hop - 1], [8 * hop, 1])
    assert model.train == 1


def test_generator_width_rule():
    from viai_amd.inpaint import generator_width_rule
    assert all(generator_width_rule(t) is None for t in (1, 2, 31, 32, 33, 208))
    assert generator_width_rule(0) is not None
    assert generator_width_rule(208, 52) is None and generator_width_rule(32, 8) is None        # N = T / 4
    assert "bottleneck" in generator_width_rule(208, 40)


def test_inpaint_waveform_gap_unit():
    from viai_amd.wavenet import inpaint_waveform
    net = make_vocoder(scales=(2, 2), cin=4)
    c = torch.rand(2, 4, 10)
    wav = torch.zeros(2, 40)
    with pytest.raises(ValueError, match="gap_unit"):
        inpaint_waveform(net, wav, c, [2, 3], [1, 1], gap_unit="seconds")
    with pytest.raises(ValueError, match="inside the clip's 40 samples"):
        inpaint_waveform(net, wav, c, [2, 39], [1, 2], gap_unit="samples")
    with pytest.raises(ValueError, match="inside the clip's 10 frames"):               # the default is today's call, message included
        inpaint_waveform(net, wav, c, [2, 9], [1, 2])
    with pytest.raises(ValueError, match="inside the clip's 10 frames"):
        inpaint_waveform(net, wav, c, [2, 9], [1, 2], gap_unit="frames")
    with pytest.raises(ValueError, match="frames"):
        inpaint_waveform(net, torch.zeros(2, 41), c, [2, 3], [1, 1], gap_unit="samples")   # n != frames * hop in either unit


def test_new_symbols_are_exported_and_typed():
    from viai_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "viai_hip.h")) as f:
        header = f.read()
    for name in NEW:
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == 8, name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == list(args)
        assert ("int %s(" % name) in header
    inval, one = 1, 16                                    # hipErrorInvalidValue; a stand-in for a device pointer that is never followed
    assert lib.viai_gap_frame_mask(one, one, one, 1, 8, 4, 0, None) == inval          # hop < 1
    assert lib.viai_gap_frame_mask(one, one, None, 1, 8, 4, 2, None) == inval
    assert lib.viai_gap_frame_mask(one, one, 18, 1, 8, 4, 2, None) == inval           # not a float pointer
    assert lib.viai_wav_align(one, one, one, one, 1, 8, -1, None) == inval            # lpad < 0
    assert lib.viai_wav_align(one, one, one, one, 0, 8, 4, None) == inval
    assert lib.viai_mel_compose(one, one, one, one, 1, 0, 8, None) == inval           # F < 1
    assert lib.viai_mel_compose(one, None, one, one, 1, 4, 8, None) == inval


def test_the_package_exports_the_inpainter():
    import viai_amd
    from viai_amd import inpaint
    assert viai_amd.AudioInpainter is inpaint.AudioInpainter and viai_amd.gap_frames is inpaint.gap_frames
    with pytest.raises(AttributeError):
        viai_amd.no_such_name
