"""GPU: sample-by-sample synthesis of the one-hot (softmax) WaveNet, `WaveNet(scalar_input=False).incremental_forward`, against the reference's
own incremental_forward (tests/golden/wavenet_onehot_synth.npz, tools/make_goldens.py wavenet_onehot_synth_goldens) in the three modes of
wavenet.py:350-356, both chain forms (VIAI_WN_FUSED), and against the library's own invariants (batch forward, streams, input forms, graphs)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import viai_oracle as O
from oracle import wavenet_oracle as W


class WNConfigOneHotDeep(W.WNConfigDeep):
    """the reference's depth (24 layers, dilations 1 .. 32 four times: every ring wraps within T = 160) with one-hot input, 256 classes"""
    out_channels = 256
    scalar_input = False


class WNConfigOneHotG(W.WNConfigOneHot):
    """the small one-hot network with global (speaker) conditioning"""
    gin_channels = 8
    n_speakers = 3


NETS = {"small": (W.WNConfigOneHot, "WN."), "deep": (WNConfigOneHotDeep, "WNOD.")}


def relerr(a, b):
    a = torch.as_tensor(a).detach().double().cpu().reshape(-1)
    b = torch.as_tensor(b).detach().double().cpu().reshape(-1)
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "wavenet_onehot_synth.npz"))


def make_net(cfg, tag, gains=(1.0, 1.0), scalar_input=False):
    from viai_amd.wavenet import WaveNet
    net = WaveNet(out_channels=cfg.out_channels, layers=cfg.layers, stacks=cfg.stacks, residual_channels=cfg.residual_channels,
                  gate_channels=cfg.gate_channels, skip_out_channels=cfg.skip_out_channels, kernel_size=cfg.kernel_size, dropout=0.0,
                  cin_channels=cfg.cin_channels, gin_channels=cfg.gin_channels, n_speakers=cfg.n_speakers, weight_normalization=True,
                  upsample_conditional_features=True, upsample_scales=list(cfg.upsample_scales), freq_axis_kernel_size=cfg.freq_axis_kernel_size,
                  scalar_input=scalar_input)
    sd = W.wavenet_state(cfg, tag)
    # the fixture's sharpened distribution (see the generator): what is fed back must matter
    sd["first_conv.weight_g"] = sd["first_conv.weight_g"] * float(gains[0])
    sd["last_conv_layers.3.weight_g"] = sd["last_conv_layers.3.weight_g"] * float(gains[1])
    assert list(net.state_dict().keys()) == list(sd.keys())
    net.load_state_dict(sd)
    return net.cuda().eval()


def case(name, gold):
    """network and the closed-form inputs of the fixture: conditioning c (B, cin, T / 16), one-hot teacher-forced input x (B, K, T), the B = 1 uniforms"""
    cfg, tag = NETS[name]
    B, T, K, stride, utag = (int(v) for v in gold[name + ".meta"])
    net = make_net(cfg, tag, gold[name + ".gains"])
    c = O.cf_uniform("wnos.%s.c" % name, (B, cfg.cin_channels, T // 16), 0, 1).cuda()
    idx = (O.cf_uniform("wnos.%s.idx" % name, (B, T), 0, 1) * K).long().clamp(max=K - 1)
    x = torch.nn.functional.one_hot(idx, K).float().transpose(1, 2).contiguous().cuda()
    u = O.cf_uniform("wnos.%s.u%d" % (name, utag), (1, T), 0, 1).cuda()
    return net, c, x, u, T, K, stride


def cdf_err(p, ref):
    """largest absolute difference between the CDFs of two sets of probabilities (B, K, n), fp64"""
    a, b = (np.cumsum(np.asarray(v.cpu() if torch.is_tensor(v) else v, dtype=np.float64), axis=1) for v in (p, ref))
    return float(np.abs(a / a[:, -1:] - b / b[:, -1:]).max())


@pytest.mark.parametrize("fused", ["0", "1"])
@pytest.mark.parametrize("name", ["small", "deep"])
def test_teacher_forced_probabilities_and_logits_match_reference_golden(name, fused, gold, monkeypatch):
    """1. softmax=True / quantize=False and softmax=False / quantize=False with every input teacher-forced: relative L2 error < 1e-4"""
    monkeypatch.setenv("VIAI_WN_FUSED", fused)
    net, c, x, _, T, K, stride = case(name, gold)
    p = net.incremental_forward(None, c=c, T=T, test_inputs=x, softmax=True, quantize=False)
    assert tuple(p.shape) == (2, K, T)
    e_p, e_cdf = relerr(p[:, :, ::stride], gold[name + ".p_tf"]), cdf_err(p[:, :, ::stride], gold[name + ".p_tf"])
    lg = net.incremental_forward(None, c=c, T=T, test_inputs=x, softmax=False, quantize=False)
    e_l = relerr(lg[:, :, torch.from_numpy(gold[name + ".logit_steps"]).cuda()], gold[name + ".l_tf"])
    print("onehot synth %s fused=%s: probabilities %.3g, logits %.3g, largest CDF difference %.3g (smallest margin of the sampled run %.3g)"
          % (name, fused, e_p, e_l, e_cdf, gold[name + ".margins"].min()))
    assert e_p < 1e-4 and e_l < 1e-4, (e_p, e_l)


@pytest.mark.parametrize("fused", ["0", "1"])
def test_teacher_forced_incremental_equals_batch_forward(fused, gold, monkeypatch):
    """2. SURVEY section 4 (i): with every input teacher-forced the step-by-step probabilities are forward(softmax=True)'s"""
    monkeypatch.setenv("VIAI_WN_FUSED", fused)
    for name in ("small", "deep"):
        net, c, x, _, T, K, _ = case(name, gold)
        with torch.no_grad():
            want = net(x, c, softmax=True)
        got = net.incremental_forward(None, c=c, T=T, test_inputs=x, softmax=True, quantize=False)
        assert relerr(got, want) < 1e-4, (name, relerr(got, want))
        # (B, n, K) is accepted like (B, K, n)
        got2 = net.incremental_forward(None, c=c, T=T, test_inputs=x.transpose(1, 2).contiguous(), softmax=True, quantize=False)
        assert torch.equal(got, got2)


@pytest.mark.parametrize("fused", ["0", "1"])
@pytest.mark.parametrize("name", ["small", "deep"])
def test_free_running_dense_feedback_matches_reference_golden(name, fused, gold, monkeypatch):
    """3. four teacher-forced steps, then the probabilities fed back (dense form of the first conv): < 1e-3"""
    monkeypatch.setenv("VIAI_WN_FUSED", fused)
    net, c, x, _, T, K, stride = case(name, gold)
    p = net.incremental_forward(None, c=c, T=T, test_inputs=x[:, :, :4].contiguous(), softmax=True, quantize=False)
    e = relerr(p[:, :, ::stride], gold[name + ".p_free"])
    print("onehot synth %s fused=%s: free-running probabilities %.3g" % (name, fused, e))
    assert e < 1e-3, e


@pytest.mark.parametrize("fused", ["0", "1"])
@pytest.mark.parametrize("name", ["small", "deep"])
def test_sampled_run_draws_the_reference_classes_at_every_step(name, fused, gold, monkeypatch):
    """4. B = 1, quantize=True, four teacher-forced steps: the class of every step is the reference's (the fixture keeps every draw
    >= 1e-4 / 3e-5 away from the CDF's edges)"""
    monkeypatch.setenv("VIAI_WN_FUSED", fused)
    net, c, x, u, T, K, stride = case(name, gold)
    cls = net.incremental_forward(None, c=c[:1], T=T, test_inputs=x[:1, :, :4].contiguous(), softmax=True, quantize=True, uniforms=u, return_classes=True)
    assert cls.dtype == torch.int64 and tuple(cls.shape) == (1, T)
    want = torch.from_numpy(gold[name + ".classes"]).reshape(1, T)
    diff = (cls.cpu() != want).nonzero()
    assert diff.numel() == 0, "first differing step %d (margin there %.3g): got %d, reference %d" % (
        int(diff[0, 1]), gold[name + ".margins"][int(diff[0, 1])], int(cls[0, diff[0, 1]]), int(want[0, diff[0, 1]]))


def stream_inputs(B, T, K, cin):
    c = O.cf_uniform("wnos.streams.c", (8, cin, T // 16), 0, 1)[:B].contiguous().cuda()
    idx = (O.cf_uniform("wnos.streams.idx", (8, 4), 0, 1) * K).long().clamp(max=K - 1)[:B]
    x = torch.nn.functional.one_hot(idx, K).float().transpose(1, 2).contiguous().cuda()
    u = O.cf_uniform("wnos.streams.u", (8, T), 0, 1)[:B].contiguous().cuda()
    return c, x, u


@pytest.mark.parametrize("fused", ["0", "1"])
@pytest.mark.parametrize("B", [2, 4, 8])
def test_streams_are_independent(B, fused, gold, monkeypatch):
    """5. stream b of a batched sampled run is the B = 1 run on stream b's inputs and uniforms, class for class"""
    monkeypatch.setenv("VIAI_WN_FUSED", fused)
    cfg, tag = NETS["small"]
    net = make_net(cfg, tag, gold["small.gains"])
    T, K = 64, cfg.out_channels
    c, x, u = stream_inputs(B, T, K, cfg.cin_channels)
    both = net.incremental_forward(None, c=c, T=T, test_inputs=x, uniforms=u, return_classes=True)
    assert tuple(both.shape) == (B, T)
    for b in range(B):
        one = net.incremental_forward(None, c=c[b:b + 1], T=T, test_inputs=x[b:b + 1], uniforms=u[b:b + 1], return_classes=True)
        assert torch.equal(one[0], both[b]), (b, (one[0] != both[b]).nonzero()[:4])
    assert len({tuple(r.tolist()) for r in both}) == B          # and the streams do differ


@pytest.mark.parametrize("fused", ["0", "1"])
def test_class_form_and_dense_form_of_the_first_conv_agree(fused, gold, monkeypatch):
    """6. one-hot teacher-forced rows through the row gather and the same rows through the K-long product"""
    monkeypatch.setenv("VIAI_WN_FUSED", fused)
    net, c, x, u, T, K, _ = case("small", gold)
    u2 = O.cf_uniform("wnos.forms.u", (2, T), 0, 1).cuda()
    res = {}
    for form in ("auto", "dense"):
        res[form] = (net.incremental_forward(None, c=c, T=T, test_inputs=x, softmax=True, quantize=False, input_form=form),
                     net.incremental_forward(None, c=c, T=T, test_inputs=x, uniforms=u2, return_classes=True, input_form=form))
    assert relerr(res["dense"][0], res["auto"][0]) < 1e-6
    assert torch.equal(res["dense"][1], res["auto"][1])


@pytest.mark.parametrize("fused", ["0", "1"])
def test_graph_replay_and_repeat_runs_are_bitwise_equal(fused, gold, monkeypatch):
    """7. use_graph=True (time index in device memory) equals the default loop bit for bit, in the sampled and in the dense-feedback mode;
    two identical runs are bitwise equal"""
    monkeypatch.setenv("VIAI_WN_FUSED", fused)
    net, c, x, u, T, K, _ = case("deep", gold)
    c2, x2, u2 = stream_inputs(2, T, K, 80)
    run_s = lambda g: net.incremental_forward(None, c=c2, T=T, test_inputs=x2, uniforms=u2, return_classes=True, use_graph=g)
    run_d = lambda g: net.incremental_forward(None, c=c, T=T, test_inputs=x[:, :, :4].contiguous(), softmax=True, quantize=False, use_graph=g)
    s0, d0 = run_s(False), run_d(False)
    assert torch.equal(run_s(False), s0) and torch.equal(run_d(False), d0)
    assert torch.equal(run_s(True), s0) and torch.equal(run_d(True), d0)
    # free-running from the initial input (class 127, wavenet.py:308-312) and from an explicit one in either layout
    i0 = net.incremental_forward(None, c=c[:1], T=T, uniforms=u, return_classes=True)
    init = torch.zeros(1, K, 1, device="cuda")
    init[0, 127, 0] = 1
    assert torch.equal(net.incremental_forward(init, c=c[:1], T=T, uniforms=u, return_classes=True), i0)
    assert torch.equal(net.incremental_forward(init.transpose(1, 2).contiguous(), c=c[:1], T=T, uniforms=u, return_classes=True, use_graph=True), i0)


def test_global_conditioning_incremental_equals_batch_forward():
    """8. speaker-id conditioning (g_add) on a small one-hot network"""
    cfg = WNConfigOneHotG
    net = make_net(cfg, "WNOG.", (4.0, 12.0))
    B, T, K = 2, 48, cfg.out_channels
    c = O.cf_uniform("wnos.g.c", (B, cfg.cin_channels, T // 16), 0, 1).cuda()
    idx = (O.cf_uniform("wnos.g.idx", (B, T), 0, 1) * K).long().clamp(max=K - 1)
    x = torch.nn.functional.one_hot(idx, K).float().transpose(1, 2).contiguous().cuda()
    g = torch.tensor([[2], [0]], dtype=torch.long).cuda()
    with torch.no_grad():
        want = net(x, c, g, softmax=True)
        other = net(x, c, torch.tensor([[1], [1]]).cuda(), softmax=True)
    assert relerr(other, want) > 1e-3                            # the speaker matters
    for fused in ("0", "1"):
        os.environ["VIAI_WN_FUSED"] = fused
        try:
            got = net.incremental_forward(None, c=c, g=g, T=T, test_inputs=x, softmax=True, quantize=False)
        finally:
            del os.environ["VIAI_WN_FUSED"]
        assert relerr(got, want) < 1e-4, (fused, relerr(got, want))


def test_classes_one_hot_rows_and_mulaw_decode(gold):
    """9. return_classes against the (B, K, T) one-hot output; mulaw_decode against the closed form in fp64"""
    from viai_amd.wavenet import mulaw_decode
    net, c, x, u, T, K, _ = case("small", gold)
    c2, x2, u2 = stream_inputs(2, T, K, 80)
    cls = net.incremental_forward(None, c=c2, T=T, test_inputs=x2, uniforms=u2, return_classes=True)
    hot = net.incremental_forward(None, c=c2, T=T, test_inputs=x2, uniforms=u2)
    assert tuple(hot.shape) == (2, K, T) and hot.dtype == torch.float32
    assert torch.equal(hot.sum(1), torch.ones(2, T, device="cuda")) and bool(((hot == 0) | (hot == 1)).all())
    assert torch.equal(hot.argmax(1), cls)
    assert 0 <= int(cls.min()) and int(cls.max()) < K and cls.unique().numel() > 8
    for mu, k in ((255, torch.arange(256).reshape(2, 128)), (255, cls.cpu()), (63, torch.arange(64).reshape(1, 64))):
        y = 2.0 * k.double() / mu - 1.0
        want = torch.sign(y) * ((1.0 + mu) ** y.abs() - 1.0) / mu
        got = mulaw_decode(k.cuda(), mu)
        assert got.dtype == torch.float32 and tuple(got.shape) == tuple(k.shape)
        assert (got.double().cpu() - want).abs().max().item() < 1e-6
    assert float(mulaw_decode(torch.tensor([0, 255]).cuda()).abs().max()) <= 1.0


def test_refusals_and_the_mixture_network_is_routed_as_before(gold):
    """10."""
    net, c, x, u, T, K, _ = case("small", gold)
    with pytest.raises(ValueError):
        net.incremental_forward(None, c=c, T=T, test_inputs=x, softmax=False, quantize=True)
    c3 = torch.cat((c, c[:1]), 0)
    with pytest.raises(NotImplementedError):
        net.incremental_forward(None, c=c3, T=T, uniforms=torch.rand(3, T), return_classes=True)
    # default uniforms: torch.rand, one per stream and step
    a = net.incremental_forward(None, c=c, T=T, return_classes=True)
    assert tuple(a.shape) == (2, T)
    mol = make_net(W.WNConfig, "WN.", scalar_input=True)
    v1 = O.cf_uniform("wn.v1", (2, T, 10), 1e-5, 1 - 1e-5)
    v2 = O.cf_uniform("wn.v2", (2, T), 1e-5, 1 - 1e-5)
    y = mol.incremental_forward(None, c=c, T=T, uniforms=(v1, v2))
    assert tuple(y.shape) == (2, 1, T) and float(y.abs().max()) <= 1.0 and y.unique().numel() > T
