"""GPU: `viai_amd.AudioInpainter` (waveform in, waveform out) and its three kernels.  Every expectation is exact (`torch.equal`): the kernels select
and copy, the rest is a composition of calls that exist.

Sizes: clips of n = 29 * 256 = 7424 samples = 32 frames at fft 1024 / hop 256 (l = 768 silent samples in front); vocoders of 4 layers in 2 stacks
(dilations 1, 2 twice: receptive field 13), 32 / 32 / 32 channels, up-sampling 4 x 4 x 4 x 4, mixture-of-logistics (30 outputs) and one-hot (256).
NUM_MELS = 68: the encoder halves the height five times, h -> (h - 1) // 2 + 1, and AvgPool2d((3, 1)) needs 3 rows of the last map, so the generator
is legal from 65 mel bands on; 68 is the first multiple of 4 (the conditioning rows of the window gather are float4s)."""
import gc

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import viai_oracle as O
from oracle import wavenet_oracle as W

NUM_MELS, FFT, HOP = 68, 1024, 256
L_PAD = FFT - HOP
N = 29 * HOP
FRAMES = 32
R = 13
KINDS = ("mol", "onehot")
_CACHE = {}


class Voc(W.WNConfig):
    layers = 4
    stacks = 2
    residual_channels = 32
    gate_channels = 32
    skip_out_channels = 32
    cin_channels = NUM_MELS
    upsample_scales = (4, 4, 4, 4)


class VocOneHot(Voc):
    out_channels = 256
    scalar_input = False


@pytest.fixture(scope="module", autouse=True)
def release_what_the_module_holds():
    """the networks live for the module; afterwards they go, and so do the blocks they left in torch's caching allocator (later modules measure it)"""
    yield
    _CACHE.clear()
    gc.collect()
    torch.cuda.empty_cache()


def bits(t):
    return t.contiguous().view(torch.int32)


def vocoder(kind):
    if kind not in _CACHE:
        from viai_amd.wavenet import WaveNet
        cfg, tag = (Voc, "IA.") if kind == "mol" else (VocOneHot, "IAO.")
        net = WaveNet(out_channels=cfg.out_channels, layers=cfg.layers, stacks=cfg.stacks, residual_channels=cfg.residual_channels,
                      gate_channels=cfg.gate_channels, skip_out_channels=cfg.skip_out_channels, kernel_size=3, dropout=0.0, cin_channels=cfg.cin_channels,
                      weight_normalization=True, upsample_scales=list(cfg.upsample_scales), scalar_input=kind == "mol")
        sd = W.wavenet_state(cfg, tag)
        if kind == "onehot":                                                          # a sharp distribution: the conditioning must matter
            sd["first_conv.weight_g"] = sd["first_conv.weight_g"] * 4.0
            sd["last_conv_layers.3.weight_g"] = sd["last_conv_layers.3.weight_g"] * 12.0
        assert list(net.state_dict().keys()) == list(sd.keys())
        net.load_state_dict(sd)
        assert net.receptive_field == R
        _CACHE[kind] = net.cuda().eval()
    return _CACHE[kind]


def generator():
    if "model" not in _CACHE:
        from viai_amd.audio import AudioConfig, MelFrontEnd
        from viai_amd.model import AudioModel, StepConfig

        class Cfg(AudioConfig):
            num_mels = NUM_MELS
        hp = StepConfig()
        hp.cin_channels, hp.max_mel_lengths = NUM_MELS, FRAMES
        model = AudioModel(hp, device="cuda:0")
        model.load_states(O.encoder_state(), O.decoder_state(), O.disc_state())
        _CACHE["model"] = model
        _CACHE["front"] = MelFrontEnd(Cfg, device="cuda:0")
    return _CACHE["model"], _CACHE["front"]


def inpainter(kind):
    from viai_amd import AudioInpainter
    model, front = generator()
    return AudioInpainter(model, vocoder(kind), front), model, front


def clip(B, tag="ia.wav"):
    return O.cf_uniform(tag, (8, N), -0.9, 0.9)[:B].contiguous().cuda()


def draws(kind, B, L, tag="ia"):
    """the sampler's uniforms in window coordinates"""
    if kind == "mol":
        return (O.cf_uniform(tag + ".u1", (8, L, 10), 1e-5, 1 - 1e-5)[:B].contiguous().cuda(),
                O.cf_uniform(tag + ".u2", (8, L), 1e-5, 1 - 1e-5)[:B].contiguous().cuda())
    return O.cf_uniform(tag + ".u", (8, L), 0, 1)[:B].contiguous().cuda()


def frame_mask_of(a0, a1, fft, hop, frames):
    """(B, 1, 1, frames) from the host rule"""
    from viai_amd import gap_frames
    first, count = gap_frames(a0, a1, fft, hop, frames)
    m = torch.ones(len(first), 1, 1, frames)
    for b, (f, c) in enumerate(zip(first, count)):
        m[b, ..., f:f + c] = 0
    return m


def dev_i32(x):
    return torch.tensor(x, dtype=torch.int32, device="cuda")


# ----------------------------------------------------------------------------- 1. the frame mask is the host rule
@pytest.mark.parametrize("fft,hop", [(1024, 256), (8, 3)])
def test_gap_frame_mask_is_the_host_rule(fft, hop):
    from viai_amd.inpaint import gap_frame_mask
    frames, k = FRAMES, 7
    l = fft - hop
    end = frames * hop                                                   # the aligned clip's length (1024 / 256: n + l = 8192)
    rows = [(end // 3, end // 3),                                        # no gap
            (l, l + hop + hop // 3),                                     # a gap at sample 0 of the clip
            (end - hop - 1, end),                                        # a gap ending with the aligned clip
            (k * hop - 1, k * hop), (k * hop, k * hop + 1), (k * hop + 1, k * hop + 2),     # one sample, around a frame boundary
            (end // 2 - hop // 2, end),                                  # wider than the second half
            (0, 1)]                                                      # the first aligned sample
    a0, a1 = [r[0] for r in rows], [r[1] for r in rows]
    got = gap_frame_mask(dev_i32(a0), dev_i32(a1), frames, fft, hop)
    want = frame_mask_of(a0, a1, fft, hop, frames)
    assert tuple(got.shape) == (8, 1, 1, frames) and got.is_contiguous()
    assert torch.equal(got.cpu(), want)
    assert float(want[0].min()) == 1 and float(want[1:].min()) == 0      # the rows do what their comments say
    # 3 rows of 33 frames: 99 floats, the scalar tail runs; and rows whose first element is not 16-byte aligned
    got = gap_frame_mask(dev_i32(a0[1:4]), dev_i32(a1[1:4]), 33, fft, hop)
    assert torch.equal(got.cpu(), frame_mask_of(a0[1:4], a1[1:4], fft, hop, 33))


# ----------------------------------------------------------------------------- 2. the aligned waveform
@pytest.mark.parametrize("n", [1027, 1028])                              # odd: scalar loads and a tail; a multiple of 4: float4 loads
def test_wav_align_pads_zeroes_and_copies_bits(n):
    from viai_amd.inpaint import wav_align
    B, lpad = 3, L_PAD
    g = torch.Generator().manual_seed(n)
    wav = torch.randint(-2 ** 31, 2 ** 31 - 1, (B, n), generator=g, dtype=torch.int64).to(torch.int32)
    wav[wav == 0] = 1                                                    # no zero words: a zero in the output is the kernel's
    wav[0, 500] = 0x7FC12345                                             # NaN payloads travel
    wav[2, 3] = -8388607                                                 # 0xFF800001, a signalling NaN
    a0 = [lpad + 10, lpad, lpad + n - 5]
    a1 = [lpad + 301, lpad + 1, lpad + n]
    out = wav_align(wav.view(torch.float32).cuda(), dev_i32(a0), dev_i32(a1), lpad)
    assert tuple(out.shape) == (B, n + lpad)
    got = bits(out).cpu()
    want = torch.cat((torch.zeros(B, lpad, dtype=torch.int32), wav), 1)
    for b in range(B):
        want[b, a0[b]:a1[b]] = 0
    assert torch.equal(got, want)
    assert int((got[:, :lpad] != 0).sum()) == 0 and all(int((got[b, a0[b]:a1[b]] != 0).sum()) == 0 for b in range(B))
    assert int((got == 0).sum()) == B * lpad + sum(y - x for x, y in zip(a0, a1))       # and nothing else is zero


# ----------------------------------------------------------------------------- 3. the composite is a select
@pytest.mark.parametrize("B,F,T,offset", [(2, 5, 37, 0), (2, 80, 208, 0), (2, 5, 37, 1)])
def test_mel_compose_is_torch_where_on_the_bits(B, F, T, offset):
    """offset 1: inputs one word off the 16-byte grid (scalar loads)"""
    from viai_amd.inpaint import mel_compose
    g = torch.Generator().manual_seed(F * T + offset)

    def pattern():
        flat = torch.randint(-2 ** 31, 2 ** 31 - 1, (B * F * T + offset,), generator=g, dtype=torch.int64).to(torch.int32)
        flat[3 + offset] = 0x7FC00001                                    # quiet and signalling NaNs, both signs of zero, an infinity
        flat[4 + offset] = 0x7F800001
        flat[5 + offset] = -2 ** 31
        flat[6 + offset] = 0
        flat[7 + offset] = 0x7F800000
        return flat.cuda()[offset:].view(B, 1, F, T)
    real, fake = pattern(), pattern()
    fake = (fake ^ 0x00400000) if offset == 0 else fake                  # NaN payloads differ between the two where both are NaN
    assert int((real != fake).sum()) > B * F * T - 8
    mask = (torch.rand(B, 1, 1, T, generator=g) < 0.5).float().cuda()
    mask[0, ..., 0], mask[0, ..., T - 1], mask[B - 1, ..., T - 1] = 0, 1, 0
    c = mel_compose(real.view(torch.float32), fake.view(torch.float32), mask)
    assert tuple(c.shape) == (B, F, T) and c.dtype == torch.float32
    want = torch.where(mask != 0, real, fake)[:, 0]
    assert torch.equal(bits(c), want)


# ----------------------------------------------------------------------------- 4. end to end
GAPS = ([1000, 2560], [301, 512])                                        # samples: [1000, 1301) and [2560, 3072)


def by_hand(kind, wav, gs, gl, uniforms):
    """the composition the inpainter stands for, out of the public pieces and torch"""
    from viai_amd.wavenet import inpaint_waveform
    model, front = generator()
    B = wav.size(0)
    a0 = [s + L_PAD for s in gs]
    a1 = [s + L_PAD + k for s, k in zip(gs, gl)]
    zeroed = wav.clone()
    for b in range(B):
        zeroed[b, gs[b]:gs[b] + gl[b]] = 0
    mask = frame_mask_of(a0, a1, FFT, HOP, FRAMES).cuda()
    mel = front(zeroed, mask)
    was, model.train = model.train, 0
    model.set_inputs(mel, mask=mask)
    fake = model.test().clone()
    model.train = was
    c = torch.where(mask != 0, mel, fake)[:, 0].contiguous()
    aligned = torch.cat((torch.zeros(B, L_PAD, device="cuda"), zeroed), 1)
    out = inpaint_waveform(vocoder(kind), aligned, c, a0, gl, uniforms=uniforms, gap_unit="samples")
    return out[:, L_PAD:], {"mask": mask, "mel": mel, "fake": fake, "c": c, "aligned": aligned}


@pytest.mark.parametrize("kind", KINDS)
def test_end_to_end_is_the_hand_written_composition(kind):
    from viai_amd import gap_frames
    inp, model, _ = inpainter(kind)
    B = 2
    gs, gl = GAPS
    wav = clip(B)
    u = draws(kind, B, R + max(gl))
    model.train = 1
    out, parts = inp(wav, gs, gl, uniforms=u, return_parts=True)
    assert model.train == 1
    out = out.clone()
    parts = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in parts.items()}
    assert tuple(out.shape) == (B, N) and tuple(parts["c"].shape) == (B, NUM_MELS, FRAMES) and tuple(parts["aligned"].shape) == (B, N + L_PAD)
    want, ref = by_hand(kind, wav, gs, gl, u)
    for k in ("mask", "mel", "fake", "c", "aligned"):
        assert torch.equal(bits(parts[k]), bits(ref[k])), k
    assert torch.equal(bits(out), bits(want))
    a0 = [s + L_PAD for s in gs]
    a1 = [s + L_PAD + k for s, k in zip(gs, gl)]
    first, count = gap_frames(a0, a1, FFT, HOP, FRAMES)
    assert parts["frames"] == (first, count) and first == [3, 10] and count == [6, 5]     # wider than the gaps' own frames 6 .. 8 and 13 .. 14
    for b in range(B):
        inside = torch.zeros(N, dtype=torch.bool, device="cuda")
        inside[gs[b]:gs[b] + gl[b]] = True
        assert torch.equal(bits(out[b])[~inside], bits(wav[b])[~inside])                  # every sample outside the gap has the input's bits
        assert int((out[b][inside] != wav[b][inside]).sum()) > gl[b] // 2                 # and the gap was regenerated
        hole = parts["mask"][b, 0, 0] == 0
        assert hole.nonzero().flatten().tolist() == list(range(first[b], first[b] + count[b]))
        assert torch.equal(parts["mask"][b, 0, 0][~hole], torch.ones(FRAMES - count[b], device="cuda"))


# ----------------------------------------------------------------------------- 5. the conditioning reaches the vocoder; the gap's samples do not
@pytest.mark.parametrize("kind", KINDS)
def test_generator_reaches_the_gap_and_the_gap_samples_reach_nothing(kind):
    inp, model, _ = inpainter(kind)
    B = 2
    gs, gl = GAPS
    wav = clip(B)
    u = draws(kind, B, R + max(gl))
    base, parts = inp(wav, gs, gl, uniforms=u, return_parts=True)
    base, first = base.clone(), {k: parts[k].clone() for k in ("mask", "mel", "fake", "c", "aligned")}
    c0 = first["c"]
    # The three-frame rule.  Every frame the mask calls clean carries the mel of the UNDAMAGED clip, bit for bit: its window reads no sample of the
    # gap.  The frames in front of the gap's own do read silenced samples (their mel differs from the undamaged clip's), so a mask as wide as the
    # gap's own frames would condition the vocoder on them as if they were real; this is the assertion such a join fails.
    front = inp.front
    whole, silenced = front(wav)[:, 0], front(first["aligned"][:, L_PAD:].contiguous())[:, 0]
    hole = (first["mask"][:, 0, 0] == 0)[:, None, :].expand_as(c0)
    assert torch.equal(bits(c0)[~hole], bits(whole)[~hole])
    for b in range(B):
        own = (gs[b] + L_PAD) // HOP                                     # the first frame whose hop slot holds a sample of the gap
        for j in range(own - 3, own):
            assert bool(hole[b, 0, j]) and not torch.equal(silenced[b, :, j], whole[b, :, j]), (b, j)
        assert not bool(hole[b, 0, own - 4])
    # other samples inside the gaps: the gap is silenced before anything reads it, so no trace of them is left anywhere
    other = wav.clone()
    for b in range(B):
        other[b, gs[b]:gs[b] + gl[b]] = clip(B, "ia.other")[b, gs[b]:gs[b] + gl[b]] + 0.05
    assert int((other != wav).sum()) == sum(gl)
    again, parts = inp(other, gs, gl, uniforms=u, return_parts=True)
    for k in first:
        assert torch.equal(bits(parts[k]), bits(first[k])), k
    assert torch.equal(bits(again), bits(base))
    # one generator weight: the samples inside the gaps change, nothing else does
    bias = model.Mel_Decoder.conv6_2.bias
    kept = bias.detach().clone()
    try:
        with torch.no_grad():
            bias.add_(1.0)
        model.weights_changed()
        moved, parts = inp(wav, gs, gl, uniforms=u, return_parts=True)
        moved, c1 = moved.clone(), parts["c"].clone()
    finally:
        with torch.no_grad():
            bias.copy_(kept)
        model.weights_changed()
    assert torch.equal(bits(c1)[~hole], bits(c0)[~hole]) and int((c1[hole] != c0[hole]).sum()) > 0
    for b in range(B):
        inside = torch.zeros(N, dtype=torch.bool, device="cuda")
        inside[gs[b]:gs[b] + gl[b]] = True
        assert torch.equal(bits(moved[b])[~inside], bits(base[b])[~inside])
        assert int((moved[b][inside] != base[b][inside]).sum()) > 0, b


# ----------------------------------------------------------------------------- 6. no gap, no change
@pytest.mark.parametrize("kind", KINDS)
def test_no_gap_returns_the_waveform(kind):
    inp, _, _ = inpainter(kind)
    wav = clip(2)
    out, parts = inp(wav, [1000, 0], 0, uniforms=draws(kind, 2, R), return_parts=True)
    assert torch.equal(bits(out), bits(wav))
    assert parts["frames"] == ([0, 0], [0, 0]) and float(parts["mask"].min()) == 1
    assert torch.equal(bits(parts["c"]), bits(parts["mel"][:, 0]))


# ----------------------------------------------------------------------------- 7. the sample unit
@pytest.mark.parametrize("kind", KINDS)
def test_gaps_in_samples_equal_gaps_in_frames_where_both_can_say_it(kind):
    from viai_amd.wavenet import inpaint_waveform
    net = vocoder(kind)
    B = 2
    wav = torch.cat((clip(B), clip(B, "ia.more")[:, :L_PAD]), 1)                          # 32 frames of samples
    c = O.cf_uniform("ia.c", (B, NUM_MELS, FRAMES), 0, 1).cuda()
    f0, fl = [5, 20], [2, 1]
    u = draws(kind, B, R + 2 * HOP, "ia7")
    frames = inpaint_waveform(net, wav, c, f0, fl, uniforms=u)
    same = inpaint_waveform(net, wav, c, f0, fl, uniforms=u, gap_unit="frames")
    samples = inpaint_waveform(net, wav, c, [f * HOP for f in f0], [f * HOP for f in fl], uniforms=u, gap_unit="samples")
    assert torch.equal(bits(frames), bits(same)) and torch.equal(bits(frames), bits(samples))
    assert int((frames != wav).sum()) > HOP                                               # something was generated
    # and a gap no frame count can express moves with its start, sample by sample
    odd = inpaint_waveform(net, wav, c, [5 * HOP + 1, 20 * HOP], [2 * HOP, HOP], uniforms=u, gap_unit="samples")
    assert torch.equal(bits(odd[0, :5 * HOP + 1]), bits(wav[0, :5 * HOP + 1])) and torch.equal(bits(odd[0, 7 * HOP + 1:]), bits(wav[0, 7 * HOP + 1:]))
    assert torch.equal(bits(odd[1]), bits(samples[1]))
