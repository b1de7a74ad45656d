"""GPU: the polyphase resampler (`viai_amd.wav_resample`, csrc/wav_resample.hip) against the fp64 restatement of tests/wav_resample_common.py, and
`inpaint_at_rate` against the composition it stands for.

Tolerance of a value: |y - ref| <= (T + 4) 2^-24 sum_j |x_j| |h_j|, the forward error bound of a T-term fp32 dot product in any order (gamma_T, with
room for the products' own rounding); the restatement runs on the library's fp32 taps, so the taps' rounding is on neither side.  Where the sum of
magnitudes is zero the output must be exactly zero.  Everything about windows, batches and repeats is exact (`torch.equal` on the bits).

End to end: the small generator, front end (68 mel bands, 32 frames) and 4-layer vocoders of tests/test_inpaint_audio_gpu.py."""
import gc

import numpy as np
import pytest
import torch

import wav_resample_common as R

pytestmark = pytest.mark.gpu

from oracle import viai_oracle as O
from oracle import wavenet_oracle as W

SENTINEL = 0x7FC12345                                                    # a NaN with a payload: arithmetic on it would not keep the bits
_CACHE = {}


def bits(t):
    return t.contiguous().view(torch.int32)


def resampler(rates):
    from viai_amd.wav_resample import Resampler
    if rates not in _CACHE:
        rs = Resampler(*rates)
        taps, _ = rs.host_table()
        _CACHE[rates] = (rs, np.ascontiguousarray(taps.numpy().T.astype(np.float64)))          # (L, T) in period order, the fp32 taps as doubles
    return _CACHE[rates]


def reference(rates, x, m=None):
    rs, h = resampler(rates)
    return R.resample(x, rs.L, rs.M, rs.H, h, m)


def check_values(rates, got, x, m=None):
    """got (m,) float32 from the device against the restatement of the clip x (its true length); returns the largest error over its bound"""
    rs, _ = resampler(rates)
    want, mags = reference(rates, x, m)
    got = got.detach().cpu().numpy().astype(np.float64)
    assert got.shape == want.shape
    bound = (rs.T + 4) * 2.0 ** -24 * mags
    err = np.abs(got - want)
    assert np.all(err <= bound), (rates, float((err - bound).max()), int(np.argmax(err - bound)))
    assert np.all(got[mags == 0] == 0)
    return float((err / np.maximum(bound, 1e-300)).max())


def sentinel(B, m):
    return torch.full((B, m), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)


@pytest.fixture(scope="module", autouse=True)
def release_what_the_module_holds():
    yield
    _CACHE.clear()
    gc.collect()
    torch.cuda.empty_cache()


# ----------------------------------------------------------------------------- 1. values, all six ratios
@pytest.mark.parametrize("rates", list(R.RATIOS))
def test_values_against_the_restatement(rates):
    rs, _ = resampler(rates)
    assert (rs.L, rs.M, rs.H, rs.T) == R.RATIOS[rates]
    n = max(5 * max(rs.L, rs.M) + 7, 2 * rs.T + 5)                       # the row of ones is long enough to hold whole filters
    lengths = [1, rs.T - 3, 5 * max(rs.L, rs.M) + 7, n]
    rng = np.random.default_rng(rs.L * 1000 + rs.M)
    buf = np.full((4, n + 13), np.nan, dtype=np.float32)                 # rows longer than any length, NaN behind the lengths: read, it would show
    clips = []
    for b, ln in enumerate(lengths):
        clips.append(np.ones(ln, dtype=np.float32) if b == 3 else rng.uniform(-1, 1, ln).astype(np.float32))
        buf[b, :ln] = clips[b]
    dev = torch.from_numpy(buf).cuda()
    wav = dev[:, :n]                                                     # a view: the row stride is n + 13
    y = rs(wav, lengths=lengths)
    m = rs.out_len(n)
    assert tuple(y.shape) == (4, m) and y.dtype == torch.float32
    worst = max(check_values(rates, y[b], clips[b], m) for b in range(4))
    # the row of ones: away from the ends every output is the sum of its table row, 1 within 3e-5 (the CPU test), plus the dot product's bound;
    # a tap dropped or doubled at a period boundary would show here at the size of a tap
    k = np.arange(m)
    i0 = k * rs.M // rs.L
    inner = (i0 - rs.H >= 0) & (i0 + rs.H < n)
    dc = np.abs(y[3].cpu().numpy().astype(np.float64) - 1)
    assert inner.sum() > 0 and np.all(dc[inner] <= 3e-5 + (rs.T + 4) * 2.0 ** -24 * reference(rates, clips[3], m)[1][inner])
    print("%s: largest error over its bound %.3f" % (rates, worst))


def test_table_on_the_device_and_values_against_the_restatements_own_taps():
    """the table the kernel reads is the one `host_table()` returns, and that is the restatement's rounded to fp32 (one ulp); then one ratio against
    the restatement on its OWN fp64 taps, at the bound that has room for the taps' rounding"""
    rates = (44100, 16000)
    rs, _ = resampler(rates)
    n = 5 * rs.M + 7
    x = np.random.default_rng(11).uniform(-1, 1, n).astype(np.float32)
    y = rs(torch.from_numpy(x)[None].cuda())[0]
    taps, first = rs.host_table()
    assert tuple(rs._taps.shape) == (rs.T, rs.L) and torch.equal(bits(rs._taps).cpu(), bits(taps))
    assert torch.equal(rs._first.cpu(), first)
    h64, first64 = R.table(*rates)
    rounded = h64.astype(np.float32)
    assert np.all(np.abs(taps.numpy().T.astype(np.float64) - rounded.astype(np.float64)) <= np.spacing(np.abs(rounded)).astype(np.float64))
    assert np.array_equal(first.numpy(), first64)
    want, mags = R.resample(x, rs.L, rs.M, rs.H, h64)
    assert np.all(np.abs(y.cpu().numpy().astype(np.float64) - want) <= (rs.T + 4) * 2.0 ** -24 * mags)


# ----------------------------------------------------------------------------- 1b. views: what lies behind a row's n samples is not the clip
@pytest.mark.parametrize("rates", [(44100, 16000), (16000, 48000)])
def test_views_of_wider_rows_read_nothing_behind_the_clip(rates):
    rs, _ = resampler(rates)
    n = 3000
    g = torch.Generator().manual_seed(17)
    buf = torch.full((3, n + 40), float("nan"))
    buf[:, 20:20 + n] = torch.rand(3, n, generator=g) * 2 - 1
    dev = buf.cuda()
    view = dev[:, 20:20 + n]                                             # NaN in front of and behind every row, row stride n + 40
    assert view.stride(0) == n + 40 and not view.is_contiguous()
    plain = rs(view.contiguous())
    assert not bool(torch.isnan(plain).any())
    assert torch.equal(bits(rs(view)), bits(plain))
    more = rs.out_len(n) + 200
    assert torch.equal(bits(rs(view, out_len=more)), bits(rs(view.contiguous(), out_len=more)))
    assert torch.equal(bits(rs(view, window=(5, 900))), bits(rs(view.contiguous(), window=(5, 900))))
    # lengths on the device beyond n are cut at n
    big = torch.tensor([n + 40, n, 10], dtype=torch.int32, device="cuda")
    assert torch.equal(bits(rs(view, lengths=big)), bits(rs(view.contiguous(), lengths=[n, n, 10])))
    assert torch.equal(bits(rs(view.contiguous(), lengths=big)), bits(rs(view.contiguous(), lengths=[n, n, 10])))
    # a row repeated by expand is a valid input
    one = view[:1].contiguous()
    assert torch.equal(bits(rs(one.expand(3, n))), bits(rs(one).expand(3, -1)))
    # a resampler bound to a device takes clips there
    from viai_amd.wav_resample import Resampler
    bound = Resampler(*rates, device="cuda")
    assert bound.device == view.device and torch.equal(bits(bound(view)), bits(plain))


# ----------------------------------------------------------------------------- 2. edges: short clips, several tiles, a length inside a tile
@pytest.mark.parametrize("rates,n", [((44100, 16000), 6000), ((48000, 16000), 4000), ((16000, 48000), 700), ((22050, 16000), 6001),
                                     ((300, 1), 20000)])                 # L = 1 and a halo that fits only one period per pass
def test_short_clips_and_rows_that_end_inside_a_tile(rates, n):
    rs, _ = resampler(rates)
    m = rs.out_len(n)
    lengths = [n, 1, 10, n - n // 3, 0]                                  # several tiles; n = 1; shorter than the filter; ends inside a tile; empty
    rng = np.random.default_rng(n)
    buf = np.full((5, n), np.nan, dtype=np.float32)
    clips = [rng.uniform(-1, 1, ln).astype(np.float32) for ln in lengths]
    for b, c in enumerate(clips):
        buf[b, :len(c)] = c
    y = rs(torch.from_numpy(buf).cuda(), lengths=torch.tensor(lengths, dtype=torch.int32, device="cuda"))
    for b in range(5):
        check_values(rates, y[b], clips[b], m)
    assert int((y[4] != 0).sum()) == 0
    # a clip of one sample without `lengths`: m = ceil(L / M) outputs
    one = rs(torch.tensor([[0.75]], device="cuda"))
    assert tuple(one.shape) == (1, rs.out_len(1))
    check_values(rates, one[0], np.array([0.75], dtype=np.float32))


# ----------------------------------------------------------------------------- 3. a window of outputs written into an existing tensor
@pytest.mark.parametrize("rates,n", [((16000, 44100), 2212), ((44100, 16000), 12000), ((48000, 16000), 7000)])
def test_window_writes_its_outputs_and_nothing_else(rates, n):
    rs, _ = resampler(rates)
    L = rs.L
    m = rs.out_len(n)
    x = (torch.rand(6, n, generator=torch.Generator().manual_seed(n)) * 2 - 1).cuda()
    full = rs(x)
    windows = [(L, L + 1000), (100, 2 * L + (0 if L > 100 else 400)), (500, 500), (m + 5, m + 900), (-5, 10), (m - 3, m + 40)]
    w0, w1 = [w[0] for w in windows], [w[1] for w in windows]
    out = sentinel(6, m + 3)                                             # wider than m: the columns behind m stay as they are too
    got = rs(x, out=out, window=(w0, w1))
    assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (6, m)
    for b, (a, e) in enumerate(windows):
        a, e = max(a, 0), min(max(e, 0), m)
        inside = torch.zeros(m + 3, dtype=torch.bool, device="cuda")
        if e > a:
            inside[a:e] = True
        assert torch.equal(bits(out[b])[:m][inside[:m]], bits(full[b])[inside[:m]]), b
        assert bool((bits(out[b])[~inside] == SENTINEL).all()), b
    # one window for every row, as ints; without `out` the rest is zeros
    alone = rs(x, window=(L, 3 * L + 1))
    assert torch.equal(bits(alone[:, L:3 * L + 1]), bits(full[:, L:3 * L + 1]))
    assert int((alone[:, :L] != 0).sum()) == 0 and int((alone[:, 3 * L + 1:] != 0).sum()) == 0
    # and under `lengths`
    lengths = [n, n // 2, 1, n, 7, n - 1]
    ragged = rs(x, lengths=lengths)
    out = sentinel(6, m)
    rs(x, lengths=lengths, out=out, window=(w0, w1))
    for b, (a, e) in enumerate(windows):
        a, e = max(a, 0), min(max(e, 0), m)
        assert torch.equal(bits(out[b, a:e]), bits(ragged[b, a:e])), b


# ----------------------------------------------------------------------------- 4. a row's bits do not depend on its company
@pytest.mark.parametrize("rates", [(44100, 16000), (16000, 44100), (48000, 16000)])
def test_row_alone_in_a_batch_and_repeated(rates):
    rs, _ = resampler(rates)
    n = 9000
    x = (torch.rand(5, n, generator=torch.Generator().manual_seed(3)) * 2 - 1).cuda()
    batch = rs(x)
    assert torch.equal(bits(rs(x)), bits(batch))
    for b in (0, 3, 4):
        assert torch.equal(bits(rs(x[b:b + 1])), bits(batch[b:b + 1])), b
    assert torch.equal(bits(rs(x[1:4])), bits(batch[1:4]))
    lengths = [n, 4000, n, 17, n]
    ragged = rs(x, lengths=lengths)
    for b in (1, 3):
        assert torch.equal(bits(rs(x[b:b + 1, :lengths[b]], out_len=rs.out_len(n))), bits(ragged[b:b + 1])), b


# ----------------------------------------------------------------------------- 5. asking for more outputs pads with zeros in the same pass
@pytest.mark.parametrize("rates,n", [((44100, 16000), 20400), ((16000, 22050), 1000)])
def test_out_len_pads_with_exact_zeros(rates, n):
    rs, _ = resampler(rates)
    m = rs.out_len(n)
    x = (torch.rand(2, n, generator=torch.Generator().manual_seed(n)) * 2 - 1).cuda()
    plain = rs(x)
    more = -(-(m + 300) // 256) * 256
    padded = rs(x, out_len=more)
    assert tuple(padded.shape) == (2, more)
    assert torch.equal(bits(padded[:, :m]), bits(plain))
    quiet = R.out_len(n + rs.H, rs.L, rs.M)                              # from here on no output reads a sample of the clip
    assert m <= quiet < more
    assert bool((bits(padded[:, quiet:]) == 0).all())                    # +0.0, bit for bit
    check_values(rates, padded[0], x[0].cpu().numpy(), more)             # in between the filter rings out as the formula says
    assert tuple(rs(x, out_len=m - 5).shape) == (2, m - 5) and torch.equal(bits(rs(x, out_len=m - 5)), bits(plain[:, :m - 5]))


# ----------------------------------------------------------------------------- 6. end to end at 48 and 44.1 kHz
NUM_MELS, FFT, HOP = 68, 1024, 256
N_LOW = 29 * HOP
FRAMES = 32
RF = 13


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
        assert net.receptive_field == RF
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


def draws(kind, B, L, tag="war"):
    """the sampler's uniforms in window coordinates"""
    if kind == "mol":
        return (O.cf_uniform(tag + ".u1", (8, L, 10), 1e-5, 1 - 1e-5)[:B].contiguous().cuda(),
                O.cf_uniform(tag + ".u2", (8, L), 1e-5, 1 - 1e-5)[:B].contiguous().cuda())
    return O.cf_uniform(tag + ".u", (8, L), 0, 1)[:B].contiguous().cuda()


@pytest.mark.parametrize("kind,rate,n,m_plain", [("mol", 48000, 22272, 7424), ("onehot", 44100, 20400, 7402)])
def test_inpaint_at_rate_is_the_composition_and_keeps_every_other_bit(kind, rate, n, m_plain):
    from viai_amd import AudioInpainter
    from viai_amd.wav_resample import Resampler, gap_at_rate, inpaint_at_rate
    model, front = generator()
    inp = AudioInpainter(model, vocoder(kind), front)
    B = 2
    gs, gl = [3000, 9000], [900, 0]
    wav = O.cf_uniform("war.wav.%d" % rate, (2, n), -0.9, 0.9).contiguous().cuda()
    down, up = Resampler(rate, 16000), Resampler(16000, rate)
    assert down.out_len(n) == m_plain
    start, length = gap_at_rate(gs, gl, down, N_LOW)
    assert length[1] == 0 and start[1] == 0 and length[0] > gl[0] * 16000 // rate          # widened; an empty gap stays empty
    u = draws(kind, B, RF + max(length))
    out, parts = inpaint_at_rate(inp, wav, rate, gs, gl, uniforms=u, return_parts=True)
    out = out.clone()
    parts = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in parts.items()}
    assert tuple(out.shape) == (B, n) and parts["low_gap"] == (start, length)
    assert tuple(parts["low"].shape) == (B, N_LOW) and tuple(parts["low_out"].shape) == (B, N_LOW) and tuple(parts["mask"].shape) == (B, 1, 1, FRAMES)
    # the composition, written out from the public pieces
    low = down(wav, out_len=N_LOW)
    assert torch.equal(bits(low), bits(parts["low"]))
    assert torch.equal(bits(low[:, :m_plain]), bits(down(wav))) and int((low[:, R.out_len(n + down.H, down.L, down.M):] != 0).sum()) == 0
    low_out = inp(low, start, length, uniforms=u)
    assert torch.equal(bits(low_out), bits(parts["low_out"]))
    want = wav.clone()
    up(low_out, out=want, window=(gs, [s + k for s, k in zip(gs, gl)]), out_len=n)
    assert torch.equal(bits(out), bits(want))
    for b in range(B):
        inside = torch.zeros(n, dtype=torch.bool, device="cuda")
        inside[gs[b]:gs[b] + gl[b]] = True
        assert torch.equal(bits(out[b])[~inside], bits(wav[b])[~inside])                   # every sample outside the gap has the input's bits
        assert gl[b] == 0 or int((out[b][inside] != wav[b][inside]).sum()) > gl[b] // 2    # and the gap was regenerated
        # outside the widened gap the inpainter copied the low-rate clip; inside it, it did not
        lo = torch.zeros(N_LOW, dtype=torch.bool, device="cuda")
        lo[start[b]:start[b] + length[b]] = True
        assert torch.equal(bits(low_out[b])[~lo], bits(low[b])[~lo])
    # the samples written into the gap are the up-sampled inpainter output, by the formula
    got = out[0, gs[0]:gs[0] + gl[0]]
    ref, mags = reference((16000, rate), low_out[0].cpu().numpy(), n)
    err = np.abs(got.cpu().numpy().astype(np.float64) - ref[gs[0]:gs[0] + gl[0]])
    assert np.all(err <= (up.T + 4) * 2.0 ** -24 * mags[gs[0]:gs[0] + gl[0]])
    # the samples inside the gap reach nothing: the widened gap covers every low-rate sample they touch
    other = wav.clone()
    other[0, gs[0]:gs[0] + gl[0]] = 0.25
    again = inpaint_at_rate(inp, other, rate, gs, gl, uniforms=u)
    assert torch.equal(bits(again), bits(out))


def test_inpaint_at_rate_on_a_clip_cut_out_of_a_longer_buffer():
    from viai_amd import AudioInpainter
    from viai_amd.wav_resample import inpaint_at_rate
    model, front = generator()
    inp = AudioInpainter(model, vocoder("mol"), front)
    n, rate = 20400, 44100                                               # 7402 low-rate samples: the padded tail reads the end of the clip
    buf = torch.full((2, n + 500), float("nan"))
    buf[:, 100:100 + n] = O.cf_uniform("war.wav.cut", (2, n), -0.9, 0.9)
    view = buf.cuda()[:, 100:100 + n]
    gs, gl = [19500, 4000], [700, 0]                                     # a gap near the end, where the widened gap and the tail meet
    u = draws("mol", 2, RF + 400)
    want, ref = inpaint_at_rate(inp, view.contiguous(), rate, gs, gl, uniforms=u, return_parts=True)
    want, low = want.clone(), ref["low"].clone()
    got, parts = inpaint_at_rate(inp, view, rate, gs, gl, uniforms=u, return_parts=True)
    assert not bool(torch.isnan(want).any()) and not bool(torch.isnan(low).any())
    assert torch.equal(bits(parts["low"]), bits(low)) and parts["low_gap"] == ref["low_gap"]
    assert torch.equal(bits(got), bits(want))


def test_the_front_ends_own_rate_calls_the_inpainter_directly():
    from viai_amd import AudioInpainter
    from viai_amd.wav_resample import inpaint_at_rate
    model, front = generator()
    inp = AudioInpainter(model, vocoder("mol"), front)
    wav = O.cf_uniform("war.wav.16", (2, N_LOW), -0.9, 0.9).contiguous().cuda()
    u = draws("mol", 2, RF + 300)
    assert torch.equal(bits(inpaint_at_rate(inp, wav, 16000, [1000, 0], [300, 0], uniforms=u)), bits(inp(wav, [1000, 0], [300, 0], uniforms=u)))


# ----------------------------------------------------------------------------- 7. the launch forms the six ratios do not reach
# R.FORMS: the consecutive form (wav_resample_kernel<1>) at tiles of 1024, 512, 256, 128 and 64 outputs, above the period limit and below it, a
# span 17 words under the LDS budget, and the period form with a single work item per block.  Each test first asks the library which form the
# plan takes, so a later change of the rule cannot move these cases onto another kernel unnoticed.  Sizes: R.value_size, a little over two tiles.
def tile_of(rs):
    pp, lt, g, _ = rs.launch_form()
    return pp * lt * g


@pytest.mark.parametrize("rates", list(R.FORMS))
def test_values_of_the_other_launch_forms(rates):
    """test_values_against_the_restatement for every plan of R.FORMS: rows of 1, T - 3 and n samples and a row of ones, NaN behind every length
    in a view of wider rows, the same bound, and the DC check on the row of ones"""
    rs, _ = resampler(rates)
    assert ((rs.L, rs.M, rs.H, rs.T), rs.launch_form()) == R.FORMS[rates]
    n, m = R.value_size(rates)
    tile = tile_of(rs)
    assert n >= 2 * rs.T + 5 and 2 * tile < m == rs.out_len(n) and m % tile != 0       # more than two tiles and a ragged one
    lengths = [1, rs.T - 3, n, n]
    rng = np.random.default_rng(rs.L * 1000 + rs.M)
    buf = np.full((4, n + 13), np.nan, dtype=np.float32)
    clips = []
    for b, ln in enumerate(lengths):
        clips.append(np.ones(ln, dtype=np.float32) if b == 3 else rng.uniform(-1, 1, ln).astype(np.float32))
        buf[b, :ln] = clips[b]
    dev = torch.from_numpy(buf).cuda()
    wav = dev[:, :n]
    assert wav.stride(0) == n + 13
    y = rs(wav, lengths=lengths)
    assert tuple(y.shape) == (4, m) and y.dtype == torch.float32
    worst = max(check_values(rates, y[b], clips[b], m) for b in range(4))
    k = np.arange(m)
    i0 = k * rs.M // rs.L
    inner = (i0 - rs.H >= 0) & (i0 + rs.H < n)
    dc = np.abs(y[3].cpu().numpy().astype(np.float64) - 1)
    assert inner.sum() > 0 and np.all(dc[inner] <= 3e-5 + (rs.T + 4) * 2.0 ** -24 * reference(rates, clips[3], m)[1][inner])
    print("%s %s: n = %d, m = %d, largest error over its bound %.3f" % (rates, rs.launch_form(), n, m, worst))


@pytest.mark.parametrize("rates", [(11025, 16000), (4001, 400), (8337, 521), (62521, 521), (300, 1)])
def test_bits_of_the_other_launch_forms(rates):
    """tiles of 1024 (above and below the period limit), 512 and 64 consecutive outputs and the period tile of four: a row alone and in a batch,
    a repeat, a window that starts and ends inside tiles, and outputs asked for beyond the clip's, all bit for bit"""
    rs, _ = resampler(rates)
    assert rs.launch_form() == R.FORMS[rates][1]
    tile = tile_of(rs)
    n, m = R.value_size(rates)
    x = (torch.rand(3, n, generator=torch.Generator().manual_seed(n)) * 2 - 1).cuda()
    batch = rs(x)
    assert tuple(batch.shape) == (3, m)
    assert torch.equal(bits(rs(x)), bits(batch))
    for b in (0, 2):
        assert torch.equal(bits(rs(x[b:b + 1])), bits(batch[b:b + 1])), b
    # windows: from inside tile 0 to inside tile 1; one output on each side of the edge between tiles 1 and 2; empty
    a, e = tile - max(1, tile // 3), tile + max(2, tile // 2)
    assert 0 < a < tile < e < 2 * tile and a % tile != 0 and e % tile != 0 and 2 * tile + 1 <= m
    windows = [(a, e), (2 * tile - 1, 2 * tile + 1), (a, a)]
    out = sentinel(3, m + 3)
    got = rs(x, out=out, window=([w[0] for w in windows], [w[1] for w in windows]))
    assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (3, m)
    for b, (w0, w1) in enumerate(windows):
        inside = torch.zeros(m + 3, dtype=torch.bool, device="cuda")
        inside[w0:w1] = True
        assert int(inside.sum()) == w1 - w0
        assert torch.equal(bits(out[b])[:m][inside[:m]], bits(batch[b])[inside[:m]]), b
        assert bool((bits(out[b])[~inside] == SENTINEL).all()), b
    # more outputs than the clip has: the same bits in front, the formula on the zero-extended clip behind, exact zeros past the filter
    quiet = R.out_len(n + rs.H, rs.L, rs.M)
    more = quiet + tile // 2 + 3
    padded = rs(x, out_len=more)
    assert tuple(padded.shape) == (3, more) and m <= quiet < more
    assert torch.equal(bits(padded[:, :m]), bits(batch))
    assert bool((bits(padded[:, quiet:]) == 0).all())
    check_values(rates, padded[0], x[0].cpu().numpy(), more)


@pytest.mark.parametrize("rates", [(330, 1), (77109, 521)])
def test_a_plan_no_tile_fits_is_refused_and_leaves_nothing_behind(rates):
    """L <= 512 and L > 512: the plan and its table exist, the call raises before any launch, `out` keeps its bits and the next call works"""
    from viai_amd._lib import ViaiLibraryError
    from viai_amd.wav_resample import Resampler
    rs = Resampler(*rates)
    assert (rs.L, rs.M, rs.H, rs.T) == R.REFUSED[rates] and rs.launch_form() == (0, 0, 0, 0)
    taps, first = rs.host_table()
    assert tuple(taps.shape) == (rs.T, rs.L) and bool(torch.isfinite(taps).all()) and abs(float(taps.double().sum()) / rs.L - 1) < 3e-5
    n = 2 * rs.M + 5
    x = (torch.rand(2, n, generator=torch.Generator().manual_seed(n)) * 2 - 1).cuda()
    out = sentinel(2, rs.out_len(n) + 3)
    with pytest.raises(ViaiLibraryError, match="viai_wav_resample failed with hipError_t 1"):
        rs(x, out=out)
    with pytest.raises(ViaiLibraryError, match="viai_wav_resample failed with hipError_t 1"):
        rs(x, out=out, window=(0, 1))
    with pytest.raises(ViaiLibraryError, match="viai_wav_resample failed with hipError_t 1"):
        rs(x)
    torch.cuda.synchronize()                                             # nothing was launched and no error is pending
    assert bool((bits(out) == SENTINEL).all())
    ok = (300, 1)
    y = resampler(ok)[0](x[:, :3000])
    torch.cuda.synchronize()
    for b in range(2):
        check_values(ok, y[b], x[b, :3000].cpu().numpy())
