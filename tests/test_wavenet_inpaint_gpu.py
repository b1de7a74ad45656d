"""GPU: teacher-forced steps chosen per stream (`incremental_forward(..., forced=)`), the window gather / splice kernels and
`inpaint_waveform`, for the scalar-input (mixture of logistics) and the one-hot network in the three chain forms: plain chain (VIAI_WN_FUSED=0),
fused chain, captured graph.  Tiny networks (6 layers in 2 stacks, dilations 1, 2, 4 twice: receptive field 29, longest ring 9; 32 / 32 / 32
channels, 8 conditioning channels, hop 4), closed-form inputs, injected uniforms.  Everything but the comparison with the batch forward is bitwise:
a masked call runs the same kernels on the same values as the prefix call it is compared with."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import viai_oracle as O
from oracle import wavenet_oracle as W


class Tiny(W.WNConfig):
    layers = 6
    stacks = 2
    residual_channels = 32
    gate_channels = 32
    skip_out_channels = 32
    cin_channels = 8
    upsample_scales = (2, 2)


class TinyOneHot(Tiny):
    out_channels = 256
    scalar_input = False


R, HOP, K = 29, 4, 256
FORMS = ("chain", "fused", "graph")
KINDS = ("mol", "onehot")
_NETS = {}


def relerr(a, b):
    a = torch.as_tensor(a).detach().double().cpu().reshape(-1)
    b = torch.as_tensor(b).detach().double().cpu().reshape(-1)
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def net_of(kind):
    if kind not in _NETS:
        from viai_amd.wavenet import WaveNet
        cfg, tag = (Tiny, "WNI.") if kind == "mol" else (TinyOneHot, "WNIO.")
        net = WaveNet(out_channels=cfg.out_channels, layers=cfg.layers, stacks=cfg.stacks, residual_channels=cfg.residual_channels,
                      gate_channels=cfg.gate_channels, skip_out_channels=cfg.skip_out_channels, kernel_size=3, dropout=0.0, cin_channels=cfg.cin_channels,
                      weight_normalization=True, upsample_scales=list(cfg.upsample_scales), scalar_input=kind == "mol")
        sd = W.wavenet_state(cfg, tag)
        if kind == "onehot":                                                          # a sharp distribution: what is fed back must matter
            sd["first_conv.weight_g"] = sd["first_conv.weight_g"] * 4.0
            sd["last_conv_layers.3.weight_g"] = sd["last_conv_layers.3.weight_g"] * 12.0
        assert list(net.state_dict().keys()) == list(sd.keys())
        net.load_state_dict(sd)
        assert net.receptive_field == R
        _NETS[kind] = net.cuda().eval()
    return _NETS[kind]


def set_form(monkeypatch, form):
    monkeypatch.setenv("VIAI_WN_FUSED", "0" if form == "chain" else "1")
    return form == "graph"


def inputs(kind, tag, B, T):
    """conditioning (B, cin, T / hop), the sampler's uniforms, given inputs for all T steps (samples (B, 1, T) / classes (B, T))"""
    c = O.cf_uniform("wni.%s.c" % tag, (8, 8, T // HOP), 0, 1)[:B].contiguous().cuda()
    if kind == "mol":
        u = (O.cf_uniform("wni.%s.u1" % tag, (8, T, 10), 1e-5, 1 - 1e-5)[:B].contiguous().cuda(),
             O.cf_uniform("wni.%s.u2" % tag, (8, T), 1e-5, 1 - 1e-5)[:B].contiguous().cuda())
        x = O.cf_uniform("wni.%s.x" % tag, (8, 1, T), -1, 1)[:B].contiguous().cuda()
    else:
        u = O.cf_uniform("wni.%s.u" % tag, (8, T), 0, 1)[:B].contiguous().cuda()
        x = (O.cf_uniform("wni.%s.k" % tag, (8, T), 0, 1) * K).long().clamp(max=K - 1)[:B].contiguous().cuda()
    return c, u, x


def u_rows(kind, u, sl):
    return (u[0][sl], u[1][sl]) if kind == "mol" else u[sl]


def as_test_inputs(kind, x, n=None):
    """the first n given inputs in the layout incremental_forward takes: (B, 1, n) samples, (B, K, n) one-hot rows; None for n == 0"""
    if n == 0:
        return None
    x = x[..., :n]
    return x if kind == "mol" else torch.nn.functional.one_hot(x, K).float().transpose(1, 2).contiguous()


def junk_where_free(kind, ti, forced):
    """what the mask does not force may hold anything"""
    ti = ti.clone()
    free = (forced == 0)
    if kind == "mol":
        ti[:, 0][free] = 7.5
    else:
        ti.transpose(1, 2)[free] = 0.25
    return ti


def synth(kind, net, c, u, T, graph, ti=None, forced=None, **kw):
    """samples (B, T) / classes (B, T)"""
    if kind == "mol":
        return net.incremental_forward(None, c=c, T=T, test_inputs=ti, uniforms=u, use_graph=graph, forced=forced, **kw)[:, 0]
    return net.incremental_forward(None, c=c, T=T, test_inputs=ti, uniforms=u, use_graph=graph, forced=forced, return_classes=True, **kw)


def start_inputs(kind, y):
    """the inputs a free run consumed: the start value (0.0 / class 127, wavenet.py:305-312), then its own outputs"""
    first = torch.zeros_like(y[:, :1]) if kind == "mol" else torch.full_like(y[:, :1], 127)
    return torch.cat((first, y[:, :-1]), 1)


def masks_of(B, T, spans):
    m = torch.zeros(B, T, dtype=torch.bool, device="cuda")
    for b, (s, e) in spans:
        m[b, s:e] = True
    return m


# ----------------------------------------------------------------------------- 1. a prefix mask is the prefix
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind,input_form", [("mol", None), ("onehot", "auto"), ("onehot", "dense")])
def test_prefix_mask_is_the_prefix(kind, input_form, form, monkeypatch):
    graph = set_form(monkeypatch, form)
    net, B, T = net_of(kind), 2, 40
    c, u, x = inputs(kind, "prefix", B, T)
    kw = {} if input_form is None else {"input_form": input_form}
    full = as_test_inputs(kind, x)
    for n in (0, 1, 5, T):
        want = synth(kind, net, c, u, T, graph, as_test_inputs(kind, x, n), **kw)
        forced = masks_of(B, T, [(b, (0, n)) for b in range(B)])
        got = synth(kind, net, c, u, T, graph, junk_where_free(kind, full, forced), forced, **kw)
        assert torch.equal(got, want), (n, (got != want).nonzero()[:4])
        if n == 5:                                                                    # uint8 like bool
            assert torch.equal(synth(kind, net, c, u, T, graph, full, forced.to(torch.uint8), **kw), want)


# ----------------------------------------------------------------------------- 2. a forced span in the middle
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind", KINDS)
def test_forced_span_equals_the_prefix_run_that_expresses_it(kind, form, monkeypatch):
    """y: the free run; yin: the inputs it consumed (step t consumes the start value at t = 0 and y[t - 1] after it).  Forcing the span [s, e) to
    other values x' must give the prefix-forced run whose first e inputs are yin[:s] followed by x' -- and must differ from y behind the span,
    which is what fails if the mask is ignored."""
    graph = set_form(monkeypatch, form)
    net, B, T = net_of(kind), 2, 48
    c, u, x = inputs(kind, "span", B, T)
    y = synth(kind, net, c, u, T, graph)
    yin = start_inputs(kind, y)
    for s in (1, 7):
        for n in (1, 4, 2 * 4 + 1):
            e = s + n
            xs = x[..., s:e]                                                          # x'
            if kind == "onehot":
                xs = torch.where(xs == yin[:, s:e], (xs + 100) % K, xs)
                prefix = torch.cat((yin[:, :s], xs), 1)
                assert not bool((xs == yin[:, s:e]).any())
            else:
                prefix = torch.cat((yin[:, :s], xs[:, 0]), 1).unsqueeze(1)
                assert not bool((xs[:, 0] == yin[:, s:e]).any())
            want = synth(kind, net, c, u, T, graph, as_test_inputs(kind, prefix))
            forced = masks_of(B, T, [(b, (s, e)) for b in range(B)])
            full = torch.zeros_like(x)
            full[..., s:e] = xs
            got = synth(kind, net, c, u, T, graph, junk_where_free(kind, as_test_inputs(kind, full), forced), forced)
            assert torch.equal(got, want), (s, e, (got != want).nonzero()[:4])
            assert torch.equal(got[:, :s], y[:, :s])
            assert all(not torch.equal(got[b, e:], y[b, e:]) for b in range(B)), (s, e)


# ----------------------------------------------------------------------------- 3. streams with different masks
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind,input_form", [("mol", None), ("onehot", "auto"), ("onehot", "dense")])
def test_streams_with_different_masks_are_independent(kind, input_form, form, monkeypatch):
    """one stream all free, one all forced, one with a span, one with a prefix and a span: at most steps the four streams' inputs come from
    different places (for the one-hot network in its dense form: some streams' from rows, others' from classes, in one launch)"""
    graph = set_form(monkeypatch, form)
    net, B, T = net_of(kind), 4, 40
    c, u, x = inputs(kind, "streams", B, T)
    kw = {} if input_form is None else {"input_form": input_form}
    forced = masks_of(B, T, [(1, (0, T)), (2, (3, 20)), (3, (0, 10)), (3, (30, 35))])
    ti = junk_where_free(kind, as_test_inputs(kind, x), forced) if input_form != "dense" else as_test_inputs(kind, x)
    both = synth(kind, net, c, u, T, graph, ti, forced, **kw)
    assert tuple(both.shape) == (B, T)
    for b in range(B):
        sl = slice(b, b + 1)
        one = synth(kind, net, c[sl], u_rows(kind, u, sl), T, graph, ti[sl], forced[sl], **kw)
        assert torch.equal(one[0], both[b]), (b, (one[0] != both[b]).nonzero()[:4])
    assert len({tuple(r.tolist()) for r in both}) == B


# ----------------------------------------------------------------------------- 4. fully forced logits against the batch forward
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind", KINDS)
def test_fully_forced_mask_meets_the_batch_forward(kind, form, monkeypatch):
    """the comparison and the tolerance of test_incremental_equals_batch_forward_under_teacher_forcing (test_wavenet_gpu.py) and
    test_teacher_forced_incremental_equals_batch_forward (test_wavenet_onehot_synth_gpu.py): relative L2 error < 1e-4"""
    graph = set_form(monkeypatch, form)
    net, B, T = net_of(kind), 2, 48
    c, u, x = inputs(kind, "full", B, T)
    forced = torch.ones(B, T, dtype=torch.bool, device="cuda")
    ti = as_test_inputs(kind, x)
    with torch.no_grad():
        if kind == "mol":
            want = net(x, c)
            _, got = net.incremental_forward(None, c=c, T=T, test_inputs=ti, uniforms=u, use_graph=graph, forced=forced, return_logits=True)
            got = got.transpose(1, 2)
        else:
            want = net(ti, c, softmax=True)
            got = net.incremental_forward(None, c=c, T=T, test_inputs=ti, softmax=True, quantize=False, use_graph=graph, forced=forced)
    e = relerr(got, want)
    print("fully forced %s %s: relative error to forward() %.3g" % (kind, form, e))
    assert e < 1e-4, e


# ----------------------------------------------------------------------------- 5. the pipelined form is not taken
def test_masked_call_at_the_reference_size_takes_the_chain(monkeypatch):
    """the pipelined kernel knows the prefix rule only: a masked call at the size and stream count it serves runs the chain, and a prefix mask
    there is the chain's prefix call bit for bit"""
    from viai_amd import wavenet_synth
    from viai_amd.wavenet import WaveNet
    monkeypatch.delenv("VIAI_WN_FUSED", raising=False)
    monkeypatch.delenv("VIAI_WN_PIPE", raising=False)
    cfg = W.WNConfigFull
    net = WaveNet(dropout=0.0)
    net.load_state_dict(W.wavenet_state(cfg, "WN."))
    net = net.cuda().eval()
    B, T = 1, 12
    c = O.cf_uniform("wni.ref.c", (B, cfg.cin_channels, T), 0, 1).cuda()                # already at the sample rate
    u = (O.cf_uniform("wni.ref.u1", (B, T, 10), 1e-5, 1 - 1e-5), O.cf_uniform("wni.ref.u2", (B, T), 1e-5, 1 - 1e-5))
    x = O.cf_uniform("wni.ref.x", (B, 1, T), -1, 1).cuda()
    forced = masks_of(B, T, [(0, (0, 5))])
    seen = []
    real = wavenet_synth._synth_form
    monkeypatch.setattr(wavenet_synth, "_synth_form", lambda *a, **k: (seen.append((a, k)), real(*a, **k))[1])
    timing = {"warmup": 0}
    got = net.incremental_forward(None, c=c, test_inputs=x, uniforms=u, forced=forced, c_upsampled=True, timing=timing)
    args = seen[-1][0]
    assert args[-1] is True and timing.get("form") != "pipe"                           # masked; and (below) the chain's result
    if args[3]:                                                                       # the device offers the pipelined form: without a mask it is taken
        assert real(*args[:-1]) == "pipe"
    monkeypatch.setenv("VIAI_WN_PIPE", "0")
    want = net.incremental_forward(None, c=c, T=T, test_inputs=x[:, :, :5].contiguous(), uniforms=u, c_upsampled=True)
    assert torch.equal(got, want) and float(got.abs().max()) > 0.01


# ----------------------------------------------------------------------------- 6. gather and splice
def np_gather(wav, cls, cond, w, ln, L, Rr, silence):
    B, n = wav.shape
    x, k = np.zeros((B, L), np.float32), np.full((B, L), silence, np.int32)
    co, forced = np.zeros((B, L, cond.shape[2]), np.float32), np.ones((B, L), np.uint8)
    for b in range(B):
        for t in range(L):
            s = w[b] + t
            if 0 <= s < n:
                x[b, t], k[b, t], co[b, t] = wav[b, s], cls[b, s], cond[b, s]
            if Rr <= t < Rr + ln[b]:
                forced[b, t] = 0
    return x, k, co, forced


def np_splice(wav, gen, g0, ln, Rr, fade):
    out = wav.copy()
    B, n = wav.shape
    for b in range(B):
        for i in range(max(g0[b], 0), min(g0[b] + ln[b], n)):
            g = gen[b, Rr + i - g0[b]]
            j = i - (g0[b] + ln[b] - fade)
            if fade > 0 and j >= 0:
                a = np.float32(j + 1) / np.float32(fade + 1)
                g = np.float32(g + np.float32(a * np.float32(wav[b, i] - g)))
            out[b, i] = g
    return out


def test_window_gather_and_splice_against_numpy():
    from viai_amd import wavenet_inpaint
    B, n, cin, Rr, frame = 4, 40, 4, 5, 4
    w = [-3, 0, 30, 12]                                                               # before the clip, at its start, running past its end, inside
    ln = [1 * frame, 3 * frame, 3 * frame, 7]                                         # one frame, the longest (twice), an odd count
    L = Rr + max(ln)
    assert w[2] + L > n
    wav = O.cf_uniform("wni.g.wav", (B, n), -1, 1)
    cls = (O.cf_uniform("wni.g.cls", (B, n), 0, 1) * K).to(torch.int32)
    cond = O.cf_uniform("wni.g.cond", (B, n, cin), 0, 1)
    x, k, co, forced = wavenet_inpaint.window_gather(w, ln, L, Rr, wav=wav.cuda(), classes=cls.cuda(), cond=cond.cuda(), silence_class=127)
    wx, wk, wco, wf = np_gather(wav.numpy(), cls.numpy(), cond.numpy(), w, ln, L, Rr, 127)
    assert x.dtype == torch.float32 and k.dtype == torch.int32 and forced.dtype == torch.uint8
    assert np.array_equal(x.cpu().numpy().view(np.uint32), wx.view(np.uint32)) and np.array_equal(k.cpu().numpy(), wk)
    assert np.array_equal(co.cpu().numpy().view(np.uint32), wco.view(np.uint32)) and np.array_equal(forced.cpu().numpy(), wf)
    assert (wx[0, :3] == 0).all() and (wk[2, n - w[2]:] == 127).all() and wf.min() == 0
    # one input alone, no conditioning: the other outputs are not produced
    x2, k2, co2, f2 = wavenet_inpaint.window_gather(w, ln, L, Rr, wav=wav.cuda())
    assert torch.equal(x2, x) and k2 is None and co2 is None and torch.equal(f2, forced)
    with pytest.raises(ValueError):
        wavenet_inpaint.window_gather(w, ln, L, Rr, wav=wav.cuda(), cond=torch.zeros(B, n, 6).cuda())
    gen = O.cf_uniform("wni.g.gen", (B, L), -1, 1)
    g0 = [v + Rr for v in w]                                                          # 2, 5, 35 (the gap runs past the clip), 17
    for fade in (0, 3):
        got = wavenet_inpaint.splice(wav.cuda(), gen.cuda(), g0, ln, Rr, fade).cpu().numpy()
        want = np_splice(wav.numpy(), gen.numpy(), g0, ln, Rr, fade)
        ulps = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
        same_sign = np.signbit(got) == np.signbit(want)
        assert int(ulps[same_sign].max()) <= (0 if fade == 0 else 1) and bool((same_sign | (np.abs(got - want) < 1e-7)).all()), fade
        outside = np.ones((B, n), bool)
        for b in range(B):
            outside[b, max(g0[b], 0):g0[b] + ln[b]] = False
        assert np.array_equal(got[outside].view(np.uint32), wav.numpy()[outside].view(np.uint32))
        assert not np.array_equal(got[~outside], wav.numpy()[~outside])


# ----------------------------------------------------------------------------- 7. inpaint_waveform
@pytest.mark.parametrize("fused", ["0", "1"])
@pytest.mark.parametrize("kind", KINDS)
def test_inpaint_waveform_equals_the_composition_from_public_pieces(kind, fused, monkeypatch):
    """two streams with gaps of different lengths: one starting at frame 0 (the receptive field in front of it is silence), one ending at the
    clip's last frame.  Outside the gaps the output is the input bit for bit; inside, stream b is the B = 1 prefix-forced incremental_forward
    over [silence-padded wav[g0 - R : g0] | len_b free steps] on the matching slice of the up-sampled conditioning and the same uniforms."""
    from viai_amd.wavenet import inpaint_waveform, mulaw_decode, mulaw_quantize
    monkeypatch.setenv("VIAI_WN_FUSED", fused)
    net, B, frames = net_of(kind), 2, 24
    n = frames * HOP
    gs, gl = [0, 20], [3, 4]
    L = R + max(gl) * HOP
    wav = O.cf_uniform("wni.inp.wav", (B, n), -0.9, 0.9).cuda()
    c = O.cf_uniform("wni.inp.c", (B, 8, frames), 0, 1).cuda()
    _, u, _ = inputs(kind, "inp", B, L)
    out, win = inpaint_waveform(net, wav, c, torch.tensor(gs), gl, uniforms=u, return_window=True)
    assert tuple(out.shape) == (B, n) and tuple(win["samples"].shape) == (B, L) and win["start"].tolist() == [g * HOP - R for g in gs]
    assert torch.equal(inpaint_waveform(net, wav, c, gs, gl, uniforms=u), out)
    cu = net._upsample(c)                                                             # (B, cin, n)
    cls = mulaw_quantize(wav) if kind == "onehot" else None
    for b in range(B):
        g0, ln = gs[b] * HOP, gl[b] * HOP
        T, lo = R + ln, g0 - R
        pad = max(-lo, 0)
        cw = torch.zeros(1, 8, T, device="cuda")
        cw[:, :, pad:] = cu[b:b + 1, :, max(lo, 0):g0 + ln]
        sl = (slice(b, b + 1), slice(0, T))
        if kind == "mol":
            prefix = torch.zeros(1, 1, R, device="cuda")
            prefix[0, 0, pad:] = wav[b, max(lo, 0):g0]
            gap = net.incremental_forward(None, c=cw, T=T, test_inputs=prefix, uniforms=(u[0][sl], u[1][sl]), c_upsampled=True)[0, 0, R:]
        else:
            pk = torch.full((1, R), 127, dtype=torch.long, device="cuda")
            pk[0, pad:] = cls[b, max(lo, 0):g0]
            hot = torch.nn.functional.one_hot(pk, K).float().transpose(1, 2).contiguous()
            gap = mulaw_decode(net.incremental_forward(None, c=cw, T=T, test_inputs=hot, uniforms=u[sl], c_upsampled=True, return_classes=True))[0, R:]
        assert torch.equal(out[b, g0:g0 + ln], gap), (b, (out[b, g0:g0 + ln] != gap).nonzero()[:4])
        assert torch.equal(out[b, :g0], wav[b, :g0]) and torch.equal(out[b, g0 + ln:], wav[b, g0 + ln:])
        assert not torch.equal(out[b, g0:g0 + ln], wav[b, g0:g0 + ln]) and gap.unique().numel() > 4
        assert torch.equal(win["samples"][b, R:R + ln], gap)
    # a fade keeps everything but the gaps' last samples
    faded = inpaint_waveform(net, wav, c, gs, gl, uniforms=u, fade=3)
    diff = (faded != out)
    for b in range(B):
        end = (gs[b] + gl[b]) * HOP
        assert not bool(diff[b, :end - 3].any()) and not bool(diff[b, end:].any()) and bool(diff[b, end - 3:end].any())


def test_inpaint_waveform_with_the_mask_of_make_time_mask():
    from viai_amd.model import make_time_mask
    from viai_amd.wavenet import gaps_from_mask, inpaint_waveform
    net, B, frames = net_of("mol"), 4, 16
    mask = make_time_mask(B, frames, 4, generator=torch.Generator().manual_seed(11))
    gs, gl = gaps_from_mask(mask)
    assert gl.tolist() == [4] * B and len(set(gs.tolist())) > 1
    wav = O.cf_uniform("wni.mask.wav", (B, frames * HOP), -0.9, 0.9).cuda()
    c = O.cf_uniform("wni.mask.c", (B, 8, frames), 0, 1).cuda()
    _, u, _ = inputs("mol", "mask", B, R + 4 * HOP)
    out = inpaint_waveform(net, wav, c, gs, gl, uniforms=u)
    known = mask[:, 0, 0, :].bool().repeat_interleave(HOP, 1).cuda()
    assert torch.equal(out[known], wav[known]) and not bool((out[~known] == wav[~known]).all())
