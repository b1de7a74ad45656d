"""GPU: the inpainting metrics (`viai_amd.metrics`, csrc/metrics.hip) against their fp64 numpy restatement (tests/metrics_common.py).

Bounds.  The kernels sum fp64 terms made from fp32 inputs; a product or difference of two floats is exact in double, so the only error of a sum is
its order: at most count * 2^-53 relative to the sum of the terms' magnitudes, 2.3e-11 for the longest sum here (200 001 terms).  Every sum is
therefore held to 1e-10 * sum |terms|, and counts are exact.  SSIM divides moments whose denominators are at least c2 = 9e-4 and shares the
window's weights with the restatement: the per-clip mean is held to 1e-9 absolute.  Determinism is bitwise.

More than 64 partials per stream (`mt_final_kernel`: lane l sums partials l, l + 64, ..., so below that every lane sums one at the most):
    test_wave_gap_stats_past_64_chunks        gaps of 131 073 and 200 001 samples of n = 210 000: 65 and 98 chunks of 2048
    test_mel_frame_stats_of_several_chunks    (F, T) = (5, 4101): 65 chunks of 64 frames; (80, 137): 3 chunks (`mel_frame_partial_kernel`'s
                                              nchunk > 1, by value)
    test_mel_ssim_past_64_tiles               (F, T) = (27, 1035) at 11 taps: 2 x 33 = 66 tiles"""
import gc
import math

import numpy as np
import pytest
import torch

import metrics_common as R

pytestmark = pytest.mark.gpu

REL = 1e-10
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def release_what_the_module_holds():
    yield
    _CACHE.clear()
    gc.collect()
    torch.cuda.empty_cache()


def uniform(seed, shape, lo=0.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * (hi - lo) + lo).float()


def check_sums(got, want, mags, what):
    """got, want, mags: one stream's row; entry 0 is a count"""
    got = got.cpu().numpy()
    assert got[0] == want[0], (what, got[0], want[0])
    for k in range(1, len(want)):
        err, bound = abs(got[k] - want[k]), REL * mags[k]
        print("%s [%d]: |gpu - ref| = %.3e, bound %.3e" % (what, k, err, bound))
        assert err <= bound, (what, k, got[k], want[k])


# ----------------------------------------------------------------------------------------------------------------------- samples of the gap
WAVE_CASES = {"edges": (1000, [(0, 1), (333, 0), (1, 999)]),                 # one sample, no gap, everything but the first sample
              "chunks": (70001, [(12345, 40001), (70000, 1)])}               # 20 chunks from an odd start with an odd length; the clip's last sample


# mt_final_kernel's lane l sums partials l, l + 64, ...: past 64 chunks (131 072 samples of a gap) a lane takes more than one
WAVE_LONG = {"65 and 98 chunks": (210000, [(777, 131073), (5, 200001)])}     # lane 0 alone takes a second chunk; lanes 0 .. 33 do


def wave_case(name):
    if ("wave", name) not in _CACHE:
        n, gaps = WAVE_CASES[name] if name in WAVE_CASES else WAVE_LONG[name]
        B = len(gaps)
        ref, est = uniform(n, (B, n), -0.9, 0.9), uniform(n + 1, (B, n), -0.9, 0.9)
        est = (0.8 * ref + 0.2 * est).float()
        want = [R.wave_gap_stats(ref[b].numpy(), est[b].numpy(), *gaps[b]) for b in range(B)]
        _CACHE[("wave", name)] = (ref.cuda(), est.cuda(), gaps, want)
    return _CACHE[("wave", name)]


@pytest.mark.parametrize("name", sorted(WAVE_CASES))
def test_wave_gap_stats(name):
    check_wave_gap_stats(name)


@pytest.mark.parametrize("name", sorted(WAVE_LONG))
def test_wave_gap_stats_past_64_chunks(name):
    n, gaps = WAVE_LONG[name]
    assert [-(-k // 2048) for _, k in gaps] == [65, 98] and all(s + k <= n for s, k in gaps)
    check_wave_gap_stats(name)


def check_wave_gap_stats(name):
    from viai_amd import metrics as M
    ref, est, gaps, want = wave_case(name)
    starts, lens = [g[0] for g in gaps], [g[1] for g in gaps]
    got = M.wave_gap_stats(ref, est, starts, lens)
    assert tuple(got.shape) == (len(gaps), 5) and got.dtype == torch.float64 and got.is_cuda
    for b, (sums, mags) in enumerate(want):
        check_sums(got[b], sums, mags, "wave %s stream %d" % (name, b))
        assert int(got[b, 0]) == lens[b]
        if lens[b] == 0:
            assert torch.equal(got[b].cpu(), torch.zeros(5, dtype=torch.float64))
    # a (B,) tensor of gaps is the same call; the derived figures are the restatement's
    again = M.wave_gap_stats(ref, est, torch.tensor(starts), torch.tensor(lens))
    assert torch.equal(again, got)
    snr, sdr = M.snr_db(got).cpu(), M.si_sdr_db(got).cpu()
    for b, (sums, _) in enumerate(want):
        if lens[b] == 0:
            assert math.isnan(float(snr[b])) and math.isnan(float(sdr[b]))
        elif lens[b] > 1:                                                    # one sample: est is a multiple of ref, SI-SDR has no distortion
            assert abs(float(snr[b]) - R.snr_db(sums)) < 1e-8 and abs(float(sdr[b]) - R.si_sdr_db(sums)) < 1e-8


def test_wave_gap_is_clamped_on_the_device_and_never_read_past():
    """the C entry point takes device-side bounds as they come: a gap that runs past the clip counts the samples inside it"""
    from viai_amd import _lib
    lib = _lib.load()
    ref, est, _, _ = wave_case("edges")
    B, n = ref.shape
    g0 = torch.tensor([990, -5, 2000], dtype=torch.int32, device="cuda")
    glen = torch.tensor([500, 10, 7], dtype=torch.int32, device="cuda")
    out = torch.full((B, 5), -1.0, dtype=torch.float64, device="cuda")
    ws = torch.empty(lib.viai_metrics_ws_doubles(0, B, n, 0, 0), dtype=torch.float64, device="cuda")
    assert lib.viai_wave_gap_stats(ref.data_ptr(), est.data_ptr(), g0.data_ptr(), glen.data_ptr(), out.data_ptr(), ws.data_ptr(), B, n,
                                   torch.cuda.current_stream().cuda_stream) == 0
    for b, (lo, hi) in enumerate(((990, 1000), (0, 5), (1000, 1000))):
        sums, mags = R.wave_gap_stats(ref[b].cpu().numpy(), est[b].cpu().numpy(), lo, hi - lo)
        check_sums(out[b], sums, mags, "clamped stream %d" % b)


# ----------------------------------------------------------------------------------------------------------------------- mel frames
def mel_masks(T):
    """(3, 1, 1, T): no damaged frame, every frame damaged, frames {0, 17, 36} damaged (those that exist)"""
    m = torch.ones(3, 1, 1, T)
    m[1] = 0
    for t in (0, 17, 36):
        if t < T:
            m[2, ..., t] = 0
    return m


def mel_case(F, T):
    if ("mel", F, T) not in _CACHE:
        ref, est = uniform(F * T, (3, 1, F, T)), uniform(F * T + 1, (3, 1, F, T))
        mask = mel_masks(T)
        want = {w: [R.mel_frame_stats(ref[b, 0].numpy(), est[b, 0].numpy(), mask[b, 0, 0].numpy(), w) for b in range(3)] for w in R.WHERE}
        _CACHE[("mel", F, T)] = (ref.cuda(), est.cuda(), mask.cuda(), want)
    return _CACHE[("mel", F, T)]


@pytest.mark.parametrize("where", R.WHERE)
@pytest.mark.parametrize("F,T", [(80, 37), (5, 1)])
def test_mel_frame_stats(F, T, where):
    check_mel_frame_stats(F, T, where)


@pytest.mark.parametrize("where", R.WHERE)
@pytest.mark.parametrize("F,T", [(80, 137), (5, 4101)])
def test_mel_frame_stats_of_several_chunks(F, T, where):
    """64 frames per block: 3 chunks, whose sum is checked for value here, and 65, where lane 0 of mt_final_kernel takes a second partial"""
    assert -(-T // 64) in (3, 65)
    check_mel_frame_stats(F, T, where)


def check_mel_frame_stats(F, T, where):
    from viai_amd import metrics as M
    ref, est, mask, want = mel_case(F, T)
    got = M.mel_frame_stats(ref, est, mask, where)
    assert tuple(got.shape) == (3, 4) and got.dtype == torch.float64
    damaged = [0, T, len([t for t in (0, 17, 36) if t < T])]
    l1, psnr, lsd = M.mel_l1(got, F).cpu(), M.mel_psnr_db(got, F).cpu(), M.mel_lsd_db(got).cpu()
    for b, (sums, mags) in enumerate(want[where]):
        check_sums(got[b], sums, mags, "mel %dx%d %s stream %d" % (F, T, where, b))
        assert int(got[b, 0]) == {"all": T, "damaged": damaged[b], "clean": T - damaged[b]}[where]
        if sums[0] == 0:                                                     # the empty clip
            assert torch.equal(got[b].cpu(), torch.zeros(4, dtype=torch.float64))
            assert math.isnan(float(l1[b])) and math.isnan(float(psnr[b])) and math.isnan(float(lsd[b]))
        else:
            assert abs(float(l1[b]) - R.mel_l1(sums, F)) < 1e-10 and abs(float(psnr[b]) - R.mel_psnr_db(sums, F)) < 1e-8
            assert abs(float(lsd[b]) - R.mel_lsd_db(sums)) < 1e-8
    if where == "all":                                                       # and without a mask
        assert torch.equal(M.mel_frame_stats(ref, est, None, "all"), got)
        assert torch.equal(M.mel_frame_stats(ref, est, where="all", min_level_db=-50)[:, :3], got[:, :3])
        assert torch.allclose(M.mel_frame_stats(ref, est, where="all", min_level_db=-50)[:, 3] * 2, got[:, 3], rtol=1e-14, atol=0)


# ----------------------------------------------------------------------------------------------------------------------- SSIM
SSIM_SHAPES = [(11, 11), (12, 300), (80, 37), (80, 259)]                     # one position; tiles along T; ragged tile edges; the native mel


def ssim_mask(T, win=11):
    """(2, 1, 1, T): damaged frames 0, 5, T - 6, T - 1 at 11 taps (win // 2 from either end in general) -- only 5 and T - 6 can be the centre of a
    window -- and, in clip 1, some more"""
    m = torch.ones(2, 1, 1, T)
    for t in (0, win // 2, T - 1 - win // 2, T - 1):
        m[:, ..., t] = 0
    m[1, ..., ::7] = 0
    return m


def ssim_case(F, T, win=11, sigma=1.5):
    key = ("ssim", F, T, win)
    if key not in _CACHE:
        from viai_amd import metrics as M
        ref = uniform(F * T + 2, (2, 1, F, T))
        est = (ref + 0.25 * (uniform(F * T + 3, (2, 1, F, T)) - 0.5)).clamp(0, 1).float()
        mask = ssim_mask(T, win)
        g = M.gaussian_window(win, sigma)                                    # the weights are shared
        assert np.abs(np.array(g) - R.gaussian(win, sigma)).max() < 2e-16
        want = {w: [R.mel_ssim(ref[b, 0].numpy(), est[b, 0].numpy(), mask[b, 0, 0].numpy(), w, g) for b in range(2)] for w in ("all", "damaged")}
        _CACHE[key] = (ref.cuda(), est.cuda(), mask.cuda(), want)
    return _CACHE[key]


def check_ssim(F, T, win, sigma):
    from viai_amd import metrics as M
    ref, est, mask, want = ssim_case(F, T, win, sigma)
    for where in ("all", "damaged"):
        got = M.mel_ssim(ref, est, mask, where, win=win, sigma=sigma)
        counts = M.mel_ssim_stats(ref, est, mask, where, win=win, sigma=sigma)[:, 0]
        assert tuple(got.shape) == (2,) and got.dtype == torch.float64
        for b, (count, mean) in enumerate(want[where]):
            print("ssim %dx%d win %d %s stream %d: gpu %.12f ref %.12f, |diff| %.3e, %d positions"
                  % (F, T, win, where, b, float(got[b]), mean, abs(float(got[b]) - mean), count))
            assert int(counts[b]) == count and count > 0
            assert abs(float(got[b]) - mean) <= 1e-9
    assert want["all"][0][0] == (F - win + 1) * (T - win + 1)
    assert want["damaged"][0][0] == (F - win + 1) * len({win // 2, T - 1 - win // 2})   # frames 0 and T - 1 are damaged and are nobody's centre
    assert torch.equal(M.mel_ssim(ref, est, None, "all", win=win, sigma=sigma), M.mel_ssim(ref, est, mask, "all", win=win, sigma=sigma))
    same = M.mel_ssim(ref, ref, None, "all", win=win, sigma=sigma)
    assert float((same - 1).abs().max()) <= 1e-12


@pytest.mark.parametrize("F,T", SSIM_SHAPES)
def test_mel_ssim(F, T):
    check_ssim(F, T, 11, 1.5)


def test_mel_ssim_past_64_tiles():
    """17 x 1025 window positions in 2 x 33 = 66 tiles of 16 x 32: lanes 0 and 1 of mt_final_kernel take a second partial"""
    F, T, win = 27, 1035, 11
    assert (-(-(F - win + 1) // 16), -(-(T - win + 1) // 32)) == (2, 33)
    check_ssim(F, T, win, 1.5)


def test_mel_ssim_with_another_window():
    check_ssim(80, 37, 7, 1.0)


def test_mel_ssim_with_the_widest_window():
    """31 taps: the largest LDS image (58 KB) and a halo wider than the tile"""
    check_ssim(48, 70, 31, 5.0)


def test_mel_ssim_counts_nothing_where_no_centre_is_selected():
    from viai_amd import metrics as M
    ref, est, _, _ = ssim_case(80, 37)
    mask = torch.ones(2, 1, 1, 37, device="cuda")
    mask[0, ..., :5] = 0                                                     # damage within win // 2 of the clip's start only
    mask[0, ..., 32:] = 0
    mask[1, ..., 20] = 0
    got = M.mel_ssim(ref, est, mask, "damaged")
    assert math.isnan(float(got[0])) and not math.isnan(float(got[1]))
    assert M.mel_ssim_stats(ref, est, mask, "damaged")[:, 0].tolist() == [0.0, 70.0]


# ----------------------------------------------------------------------------------------------------------------------- determinism
def test_results_are_bitwise_reproducible_and_independent_of_the_batch():
    from viai_amd import metrics as M
    B, n, F, T = 3, 70001, 80, 137                                           # gaps of 20, 1 and 35 chunks; 3 frame chunks; 5 x 4 SSIM tiles
    ref, est = uniform(1, (B, n), -0.9, 0.9).cuda(), uniform(2, (B, n), -0.9, 0.9).cuda()
    starts, lens = [12345, 7, 0], [40001, 2047, 70001]
    mel_r, mel_e = uniform(3, (B, 1, F, T)).cuda(), uniform(4, (B, 1, F, T)).cuda()
    mask = (uniform(5, (B, 1, 1, T)) < 0.6).float().cuda()
    calls = {
        "wave": lambda s: M.wave_gap_stats(ref[s], est[s], starts[s], lens[s]),
        "frames": lambda s: M.mel_frame_stats(mel_r[s], mel_e[s], mask[s], "damaged"),
        "frames_all": lambda s: M.mel_frame_stats(mel_r[s], mel_e[s], None, "all"),
        "ssim": lambda s: M.mel_ssim_stats(mel_r[s], mel_e[s], mask[s], "damaged"),
        "ssim_all": lambda s: M.mel_ssim_stats(mel_r[s], mel_e[s], None, "all"),
    }
    for name, call in calls.items():
        whole = call(slice(0, B)).clone()
        assert torch.equal(call(slice(0, B)), whole), name                   # run to run
        assert bool(torch.isfinite(whole).all()) and float(whole[:, 0].min()) > 0, name
        for i in range(B):
            alone = call(slice(i, i + 1))
            assert torch.equal(alone[0], whole[i]), (name, i)                # a clip alone has the bits of its row in the batch


# ----------------------------------------------------------------------------------------------------------------------- one inpainter call
NUM_MELS, FFT, HOP = 68, 1024, 256                                           # the toy sizes of tests/test_inpaint_audio_gpu.py
L_PAD, N, FRAMES = FFT - HOP, 29 * HOP, 32


def small_inpainter():
    if "inp" not in _CACHE:
        from oracle import viai_oracle as O
        from oracle import wavenet_oracle as W
        from viai_amd import AudioInpainter
        from viai_amd.audio import AudioConfig, MelFrontEnd
        from viai_amd.model import AudioModel, StepConfig
        from viai_amd.wavenet import WaveNet

        class Voc(W.WNConfig):
            layers, stacks = 4, 2
            residual_channels = gate_channels = skip_out_channels = 32
            cin_channels = NUM_MELS
            upsample_scales = (4, 4, 4, 4)

        class Cfg(AudioConfig):
            num_mels = NUM_MELS
        net = WaveNet(out_channels=Voc.out_channels, layers=Voc.layers, stacks=Voc.stacks, residual_channels=Voc.residual_channels,
                      gate_channels=Voc.gate_channels, skip_out_channels=Voc.skip_out_channels, kernel_size=3, dropout=0.0,
                      cin_channels=Voc.cin_channels, weight_normalization=True, upsample_scales=list(Voc.upsample_scales), scalar_input=True)
        net.load_state_dict(W.wavenet_state(Voc, "IA."))
        hp = StepConfig()
        hp.cin_channels, hp.max_mel_lengths = NUM_MELS, FRAMES
        model = AudioModel(hp, device="cuda:0")
        model.load_states(O.encoder_state(), O.decoder_state(), O.disc_state())
        _CACHE["inp"] = AudioInpainter(model, net.cuda().eval(), MelFrontEnd(Cfg, device="cuda:0"))
        _CACHE["O"] = O
    return _CACHE["inp"], _CACHE["O"]


def test_inpainting_report_is_the_functions_applied_by_hand():
    from viai_amd import gap_frames
    from viai_amd import metrics as M
    inp, O = small_inpainter()
    B, gs, gl = 2, [1000, 2560], [301, 512]
    wav = O.cf_uniform("ia.wav", (8, N), -0.9, 0.9)[:B].contiguous().cuda()
    L = inp.vocoder.receptive_field + max(gl)
    u = (O.cf_uniform("ia.u1", (8, L, 10), 1e-5, 1 - 1e-5)[:B].contiguous().cuda(), O.cf_uniform("ia.u2", (8, L), 1e-5, 1 - 1e-5)[:B].contiguous().cuda())
    out, parts = inp(wav, gs, gl, uniforms=u, return_parts=True)
    out = out.clone()
    parts = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in parts.items()}
    rep = M.inpainting_report(inp, wav, out, gs, gl, parts)
    assert sorted(rep) == sorted(["snr_db", "si_sdr_db", "mel_l1", "mel_psnr_db", "mel_lsd_db", "mel_ssim", "frames", "samples"])
    assert all(tuple(v.shape) == (B,) and v.dtype == torch.float64 and v.is_cuda for v in rep.values())
    # by hand: the clean clip on the inpainter's grid, its mel, and each function on the parts
    aligned = torch.cat((torch.zeros(B, L_PAD, device="cuda"), wav), 1)
    clean_mel = inp.front(aligned[:, L_PAD:])
    wave = M.wave_gap_stats(wav, out, gs, gl)
    frames = M.mel_frame_stats(clean_mel, parts["fake"], parts["mask"], "damaged", min_level_db=inp.front.cfg.min_level_db)
    want = {"snr_db": M.snr_db(wave), "si_sdr_db": M.si_sdr_db(wave), "mel_l1": M.mel_l1(frames, NUM_MELS), "mel_psnr_db": M.mel_psnr_db(frames, NUM_MELS),
            "mel_lsd_db": M.mel_lsd_db(frames), "mel_ssim": M.mel_ssim(clean_mel, parts["fake"], parts["mask"], "damaged")}
    for k, v in want.items():
        assert torch.equal(rep[k], v), k
        assert bool(torch.isfinite(v).all()), k
    assert rep["samples"].tolist() == [float(x) for x in gl]
    first, count = gap_frames([s + L_PAD for s in gs], [s + L_PAD + k for s, k in zip(gs, gl)], FFT, HOP, FRAMES)
    assert parts["frames"] == (first, count) and rep["frames"].tolist() == [float(c) for c in count]
    # the mel of a clip against itself, on the same grid, is a perfect score: the report's reference is the clean mel
    assert torch.equal(M.mel_frame_stats(clean_mel, clean_mel, parts["mask"], "damaged")[:, 1:], torch.zeros(B, 3, dtype=torch.float64, device="cuda"))
