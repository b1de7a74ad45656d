"""GPU: vocoder data preparation on the device (viai_amd.preprocess, csrc/preprocess.hip): rescaling, the silence trim, the padded signal in its
three forms, the mel on the aligned rows, and the property the stage exists for -- the training pair and `AudioInpainter`'s conditioning come
from one program and agree bit for bit.  fft 1024, hop 256, 80 bands, chunks of 4096 samples, files of 2 to 4 chunks, trimmed lengths >= fft."""
import os

import numpy as np
import pytest
import torch

from preprocess_common import mulaw_np, process_utterance_np

pytestmark = pytest.mark.gpu

FFT, HOP, MELS, CHUNK, MU = 1024, 256, 80, 4096, 255
L = FFT - HOP


def bits_equal(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return torch.equal(a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else torch.equal(a, b)


def loud(n, gen, lo=0.1, hi=0.9):
    """n samples with lo <= |x| <= hi: every one of them is active at any threshold the tests use"""
    mag = lo + (hi - lo) * torch.rand(n, generator=gen)
    return mag * (torch.randint(0, 2, (n,), generator=gen) * 2 - 1).float()


def pre(**kw):
    from viai_amd.preprocess import UtterancePreprocessor
    kw.setdefault("chunk_samples", CHUNK)
    return UtterancePreprocessor(front=front(), **kw)


_front = []


def front():
    from viai_amd.audio import AudioConfig, MelFrontEnd
    if not _front:
        _front.append(MelFrontEnd(AudioConfig, device="cuda"))
    assert (AudioConfig.fft_size, AudioConfig.hop_size, AudioConfig.num_mels) == (FFT, HOP, MELS)
    return _front[0]


def trimmed_file(gen, lengths=(8 * HOP, 8 * HOP + 1, 9 * HOP - 1), start=100, tail=50):
    """one chunk per entry: silence, `length + 1` loud samples from `start` on (the last one is the sample the exclusive end drops), silence"""
    parts = []
    for i, T in enumerate(lengths):
        c = torch.zeros(CHUNK + (tail if i == len(lengths) - 1 else 0))
        c[start:start + T + 1] = loud(T + 1, gen)
        parts.append(c)
    return torch.cat(parts)


@pytest.fixture(scope="module")
def quantized():
    """the file of `trimmed_file` through the default form: (cpu waveform, records)"""
    wav = trimmed_file(torch.Generator().manual_seed(11))
    return wav, pre(rescaling=False)(wav.cuda())


def test_rescale_is_numpys_float32_arithmetic():
    gen = torch.Generator().manual_seed(1)
    wav = torch.randn(3 * CHUNK + 77, generator=gen) * 0.3
    want = (wav / wav.abs().max()) * 0.999                               # fp32 division, fp32 multiplication, each rounded on its own
    recs = pre(input_type="raw")(wav.cuda())
    assert [r.chunk for r in recs] == [0, 1, 2] and [r.wav.numel() for r in recs] == [CHUNK, CHUNK, CHUNK + 77]
    assert bits_equal(torch.cat([r.wav for r in recs]), want)
    assert all(r.wav.data_ptr() % 16 == 0 for r in recs)
    # and the trimmed rows of the default form are slices of the same values
    wav = trimmed_file(gen) * 0.5
    want = (wav / wav.abs().max()) * 0.999
    for r in pre()(wav.cuda()):
        a = r.chunk * CHUNK
        assert (r.start, r.end) == (100, 100 + r.wav.numel()) and bits_equal(r.wav, want[a + r.start:a + r.end])


def stretch(p, n):
    """a golden class pattern on a chunk of n samples: its first three entries in front, its last one at the end, the rest in the middle"""
    out = np.full(n, 127, dtype=np.int64)
    if len(p) <= 3:
        out[:len(p)] = p
        return out
    out[:3] = p[:3]
    out[2000:2000 + len(p) - 4] = p[3:-1]
    out[n - 1] = p[-1]
    return out


def test_bounds_match_the_host_rule_on_the_devices_own_classes(golden_dir):
    from viai_amd import wavenet as W
    from viai_amd.preprocess import chunk_bounds, trim_bounds, trim_bounds_host
    g = np.load(os.path.join(golden_dir, "preprocess.npz"))
    pats = [(int(m[0]), row[:m[1]].astype(np.int64)) for row, m in zip(g["trim.classes"], g["trim.meta"])]
    seen = set()
    for thr in (0, 2, 5):
        mine = [p for t, p in pats if t == thr]
        for f0 in range(0, len(mine), 4):                                # files of 2 to 4 chunks
            group = mine[f0:f0 + 4]
            if len(group) < 2:
                group = mine[-2:]
            sizes = [CHUNK] * (len(group) - 1) + [CHUNK + 100]             # the last chunk runs to the end of the file
            cls = np.concatenate([stretch(p, n) for p, n in zip(group, sizes)])
            wav = W.mulaw_decode(torch.from_numpy(cls).int().cuda(), MU)
            chunks = chunk_bounds(wav.numel(), CHUNK)
            assert len(chunks) == len(group)
            got = trim_bounds(wav, chunks, thr, MU).cpu().tolist()
            own = W.mulaw_quantize(wav, MU).cpu().numpy()
            for (a, b), bounds in zip(chunks, got):
                assert tuple(bounds) == trim_bounds_host(own[a:b], thr), (thr, f0, a)
                s, e = bounds
                seen |= {"start0"} if s == 0 else set()
                seen |= {"last"} if e == b - a - 1 else set()
                seen |= {"only01"} if s < 2 and e == -1 else set()
                seen |= {"silent"} if s == b - a and e == -1 else set()
                seen |= {"end2"} if e == 2 else set()
    assert seen == {"start0", "last", "only01", "silent", "end2"}
    # a random signal, rescaled: silence longer than one block's span (1024 samples) in front and behind, a chunk boundary inside a silent run
    gen = torch.Generator().manual_seed(2)
    wav = torch.zeros(3 * CHUNK)
    wav[1500:CHUNK - 1300] = torch.randn(CHUNK - 2800, generator=gen) * 0.2
    wav[CHUNK + 40:2 * CHUNK - 1100] = torch.randn(CHUNK - 1140, generator=gen) * 0.2
    wav[2 * CHUNK + 1200:3 * CHUNK - 2500] = torch.randn(CHUNK - 3700, generator=gen) * 0.2
    resc = (wav / wav.abs().max()) * 0.999
    own = W.mulaw_quantize(resc.cuda(), MU).cpu().numpy()
    chunks = chunk_bounds(wav.numel(), CHUNK)
    amax = wav.abs().max().reshape(1).cuda()
    got = trim_bounds(wav.cuda(), chunks, 2, MU, amax=amax, rescaling_max=0.999).cpu().tolist()
    for (a, b), bounds in zip(chunks, got):
        assert tuple(bounds) == trim_bounds_host(own[a:b], 2), a
        assert bounds[1] < CHUNK - 1024                                      # more than one scan step of silence behind every chunk
    assert got[0][0] >= 1500 and got[1][0] >= 40 and got[2][0] >= 1200 and got[1][1] < CHUNK - 1100      # ... and in front of chunks 0 and 2
    recs = pre()(wav.cuda())
    assert [(r.start, r.end) for r in recs] == [tuple(b) for b in got]


def test_signal_mulaw_quantize(quantized):
    from viai_amd import wavenet as W
    from viai_amd.preprocess import signal_layout
    wav, recs = quantized
    assert [r.wav.numel() % HOP for r in recs] == [0, 1, HOP - 1] and all(r.wav.numel() >= FFT for r in recs)
    ref = process_utterance_np(wav.numpy(), rescaling=False, chunk=CHUNK, quantize=lambda x: W.mulaw_quantize(torch.from_numpy(x).cuda(), MU).cpu().numpy())
    assert len(ref) == len(recs) == 3
    for r, want in zip(recs, ref):
        a = r.chunk * CHUNK
        T = r.end - r.start
        l, _, N, steps = signal_layout(T, FFT, HOP)
        assert (r.chunk, r.start, r.end) == (want["chunk"], want["start"], want["end"]) == (r.chunk, 100, 100 + T)
        assert bits_equal(r.wav, wav[a + r.start:a + r.end])
        body = W.mulaw_quantize(r.wav.clone(), MU).cpu()
        expect = torch.cat([torch.full((l,), 127, dtype=torch.int32), body, torch.full((steps - l - T,), 127, dtype=torch.int32)])
        assert r.signal.dtype == torch.int32 and torch.equal(r.signal.cpu(), expect)
        assert torch.equal(r.signal.cpu(), torch.from_numpy(want["signal"]))
        assert r.timesteps == steps == N * HOP == r.mel.shape[0] * HOP == r.signal.numel()
        assert r.mel.shape == (N, MELS) and r.mel.is_contiguous() and r.mel.dtype == torch.float32


def test_signal_raw_keeps_the_bits():
    gen = torch.Generator().manual_seed(3)
    wav = torch.randn(2 * CHUNK + 131, generator=gen) * 0.25
    wav[5] = -0.0
    recs = pre(input_type="raw", rescaling=False)(wav.cuda())
    ref = process_utterance_np(wav.numpy(), "raw", rescaling=False, chunk=CHUNK)
    assert [r.wav.numel() for r in recs] == [CHUNK, CHUNK + 131]
    for r, want in zip(recs, ref):
        a = r.chunk * CHUNK
        T = r.wav.numel()
        assert (r.start, r.end) == (0, T) and r.signal.dtype == torch.float32
        expect = torch.cat([torch.zeros(L), wav[a:a + T], torch.zeros(r.timesteps - L - T)])
        assert bits_equal(r.signal, expect) and bits_equal(r.signal, torch.from_numpy(want["signal"]))


def test_signal_mulaw():
    from viai_amd import wavenet as W
    gen = torch.Generator().manual_seed(4)
    wav = (torch.rand(2 * CHUNK + 9, generator=gen) * 2 - 1) * torch.rand(2 * CHUNK + 9, generator=gen) ** 3      # many small magnitudes, some near 1
    wav[:4] = torch.tensor([0.0, 1.0, -1.0, 1e-6])
    recs = pre(input_type="mulaw", rescaling=False)(wav.cuda())
    y = torch.cat([r.signal[L:L + r.wav.numel()] for r in recs]).cpu()
    assert y.numel() == wav.numel() and all(bits_equal(r.signal[:L], torch.zeros(L)) for r in recs)
    # the class step on these floats is viai_mulaw_quantize's, exactly
    cls = torch.clamp(torch.trunc((y + 1) / 2 * MU), 0, MU).int()
    assert torch.equal(cls, W.mulaw_quantize(wav.cuda(), MU).cpu())
    # against the closed form in fp64: within four times the error of the same expression in fp32 on the CPU (torch), measured here on the
    # same inputs -- 8.15e-8 for this file, so the bound is 3.26e-7 (five and a half ulps of a value just below 1.0)
    y64 = torch.from_numpy(mulaw_np(wav.numpy(), MU))
    y32 = torch.sign(wav) * torch.log1p(MU * wav.abs()) / torch.log1p(torch.tensor(float(MU)))
    err_cpu = (y32.double() - y64).abs().max().item()
    err_dev = (y.double() - y64).abs().max().item()
    print("mulaw: fp32 torch-CPU error %.3e, device error %.3e" % (err_cpu, err_dev))
    assert 0 < err_cpu < 1e-6 and err_dev <= 4 * err_cpu


def test_mel_is_the_front_ends_on_a_fresh_copy(quantized):
    import ctypes as C
    from viai_amd import _lib
    _, recs = quantized
    fam, routes = C.create_string_buffer(32), set()
    for r in recs:
        fresh = r.wav.clone()
        assert bits_equal(r.mel, front()(fresh[None])[0, 0].t())
        assert _lib.load().viai_stft_mel_route(r.wav.numel(), FFT, HOP, MELS, int(r.wav.data_ptr() % 8 == 0), fam, 32) == 1
        routes.add((r.wav.numel() % 2, fam.value))
    assert len({f for _, f in routes}) == 2 and {p for p, _ in routes} == {0, 1}      # an even and an odd length: both routes


def test_training_pair_and_inference_conditioning_agree():
    from viai_amd import inpaint
    gen = torch.Generator().manual_seed(5)
    wav = (torch.randn(CHUNK, generator=gen) * 0.2).cuda()
    recs = pre(input_type="raw", rescaling=False)(wav)
    assert len(recs) == 1 and CHUNK % HOP == 0
    r = recs[0]
    a = torch.zeros(1, dtype=torch.int32, device="cuda")
    aligned = inpaint.wav_align(wav[None], a, a, L)                          # an empty gap
    assert bits_equal(r.signal, aligned[0])
    assert bits_equal(r.mel.t(), front()(wav[None])[0, 0])
    assert bits_equal(r.mel.t(), front()(aligned[:, L:])[0, 0])              # the view AudioInpainter hands to its front end


def test_silent_chunks_raise_or_are_skipped():
    gen = torch.Generator().manual_seed(6)
    wav = trimmed_file(gen, lengths=(5 * HOP, 6 * HOP + 3, 7 * HOP))
    full = pre(rescaling=False)(wav.cuda())
    silent = wav.clone()
    silent[CHUNK:2 * CHUNK] = 0.0                                            # class 127 throughout
    with pytest.raises(ValueError, match="chunk 1 "):
        pre(rescaling=False)(silent.cuda())
    kept = pre(rescaling=False, skip_silent=True)(silent.cuda())
    assert [r.chunk for r in kept] == [0, 2]
    for r, want in zip(kept, (full[0], full[2])):
        assert (r.start, r.end, r.timesteps) == (want.start, want.end, want.timesteps)
        assert bits_equal(r.signal, want.signal) and bits_equal(r.mel, want.mel) and bits_equal(r.wav, want.wav)
    assert pre(rescaling=False, skip_silent=True)(torch.zeros(2 * CHUNK).cuda()) == []
    with pytest.raises(ValueError):
        pre()(torch.zeros(2 * CHUNK).cuda())                                  # nothing to rescale by
    assert pre()(torch.ones(CHUNK - 1).cuda()) == []                          # shorter than one chunk: no chunk


def test_two_calls_give_the_same_bits():
    gen = torch.Generator().manual_seed(7)
    wav = trimmed_file(gen, lengths=(4 * HOP + 7, 9 * HOP)).cuda() * 0.7
    p = pre()
    one, two = p(wav), p(wav)
    assert len(one) == len(two) == 2
    for x, y in zip(one, two):
        assert (x.timesteps, x.start, x.end, x.chunk) == (y.timesteps, y.start, y.end, y.chunk)
        assert bits_equal(x.signal, y.signal) and bits_equal(x.mel, y.mel) and bits_equal(x.wav, y.wav)


def test_a_pair_trains_a_tiny_one_hot_wavenet(quantized):
    from viai_amd.wavenet import WaveNet, masked_cross_entropy
    _, recs = quantized
    r = recs[0]
    torch.manual_seed(0)
    net = WaveNet(out_channels=256, layers=4, stacks=2, residual_channels=16, gate_channels=16, skip_out_channels=16, dropout=0.0, cin_channels=MELS,
                  upsample_scales=[4, 4, 4, 4], scalar_input=False).cuda()
    rows = net.forward_nhwc(r.signal[None], r.mel.t()[None].contiguous())
    assert rows.shape[-2] == r.timesteps
    loss = masked_cross_entropy(rows, r.signal[None], shift=1, num_classes=256)
    assert torch.isfinite(loss).item() and loss.item() > 0
