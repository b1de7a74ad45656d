"""GPU: training the one-hot (mu-law, 256-way softmax) WaveNet from class indices -- the fused masked cross-entropy on NHWC rows
(`viai_masked_ce_loss`), the class form of the first layer (`viai_class_embed_fwd` / `_bwd`), `mulaw_quantize`, and both against the
reference's `WaveNet(scalar_input=False)` + `MaskedCrossEntropyLoss` (tests/golden/wavenet_onehot_train.npz, tools/make_goldens.py
--wavenet-onehot-train-only)."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import viai_oracle as O
from oracle import wavenet_oracle as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "wn_onehot_train.json")


class WNConfigOneHotFull:
    """tools/make_goldens.py's WNConfigOneHotFull, restated: the reference's size with one-hot input and 256 classes"""
    out_channels, layers, stacks, residual_channels, gate_channels, skip_out_channels = 256, 24, 4, 512, 512, 256
    kernel_size, cin_channels, upsample_scales, freq_axis_kernel_size, gin_channels, n_speakers = 3, 80, (4, 4, 4, 4), 3, -1, None
    scalar_input = False


def relerr(a, b):
    a = torch.as_tensor(a).detach().double().cpu().reshape(-1)
    b = torch.as_tensor(b).detach().double().cpu().reshape(-1)
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def build(cfg=W.WNConfigOneHot, tag="WN."):
    from viai_amd.wavenet import WaveNet
    net = WaveNet(out_channels=cfg.out_channels, layers=cfg.layers, stacks=cfg.stacks, residual_channels=cfg.residual_channels,
                  gate_channels=cfg.gate_channels, skip_out_channels=cfg.skip_out_channels, kernel_size=cfg.kernel_size, dropout=0.0,
                  cin_channels=cfg.cin_channels, gin_channels=-1, weight_normalization=True, upsample_conditional_features=True,
                  upsample_scales=list(cfg.upsample_scales), freq_axis_kernel_size=cfg.freq_axis_kernel_size, scalar_input=False)
    sd = W.wavenet_state(cfg, tag)
    assert list(net.state_dict().keys()) == list(sd.keys())
    net.load_state_dict(sd)
    return net.cuda().train()


def mulaw_vectors(mu=255):
    """tests/test_wavenet_onehot_train_cpu.py's check vectors (asserted there to sit mid-interval): decode(k + 0.5), then -1, 0, 1"""
    k = np.arange(mu, dtype=np.float64)
    y = 2.0 * (k + 0.5) / mu - 1.0
    x = np.sign(y) * np.expm1(np.abs(y) * np.log1p(mu)) / mu
    return np.concatenate([x, [-1.0, 0.0, 1.0]]), np.concatenate([np.arange(mu), [0, mu // 2, mu]]).astype(np.int64)


def ce_truth(logits_btk, target_bt, mask, shift, dtype):
    """torch on the CPU in `dtype`: masked mean of cross_entropy(row t, target t + shift), and its gradient on all T rows"""
    x = logits_btk.detach().cpu().to(dtype).requires_grad_(True)
    T = x.shape[1]
    ce = torch.nn.functional.cross_entropy(x[:, :T - shift].transpose(1, 2), target_bt.cpu().long()[:, shift:], reduction="none")
    m = mask.detach().cpu().to(dtype)
    loss = (ce * m).sum() / m.sum()
    loss.backward()
    return loss.detach(), x.grad


def record_parity(name, pairs):
    """the measured (error, bound) pairs under key `parity` of profiles/wn_onehot_train.json, beside the rate tool's figures"""
    try:
        doc = json.load(open(PROFILE)) if os.path.exists(PROFILE) else {}
        doc.setdefault("parity", {})[name] = pairs
        with open(PROFILE, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")
    except OSError:
        pass                                                    # a read-only checkout still runs the assertions


def loss_cases():
    B, T = 3, 40
    lengths = torch.tensor([T, T - 14, 9])
    for K, pitch in ((256, 256), (252, 256)):
        for shift in (0, 1):
            logits = O.cf_uniform("ce.x.%d.%d" % (K, shift), (B, T, K), -4, 4)
            sign = torch.where(O.cf_uniform("ce.s.%d.%d" % (K, shift), (2, K), 0, 1) < 0.5, -1.0, 1.0)
            logits[0, 5], logits[2, 3] = 80.0 * sign[0], 80.0 * sign[1]                 # rows of +-80: no overflow, no NaN
            logits[1, 7] = 80.0
            target = (O.cf_uniform("ce.t.%d.%d" % (K, shift), (B, T), 0, 1) * K).long().clamp(max=K - 1)
            mask = (torch.arange(T - shift).unsqueeze(0) < (lengths - shift).unsqueeze(1)).float()
            mask[0, 11:17] = 0                                                           # a hole inside a stream as well
            yield K, pitch, shift, logits, target, mask


def test_masked_ce_matches_fp64_in_every_layout():
    """1. loss and gradient (norm-wise) within 4 * e_fp32cpu + 8 * 2^-24 of torch in fp64 on the CPU, where e_fp32cpu is what torch's own
    fp32 CPU evaluation of the same inputs achieves: the three input layouts, int32 / int64 targets, shift 0 / 1, masks with whole streams
    partly zero and a hole, and K = 252 in rows of 256 with a padding gradient of exactly 0 (lengths= against mask=: the next test)."""
    from viai_amd.wavenet import MaskedCrossEntropyLoss, masked_cross_entropy
    floor = 8 * 2.0 ** -24
    pairs = {}
    for K, pitch, shift, logits, target, mask in loss_cases():
        t_loss, t_grad = ce_truth(logits, target, mask, shift, torch.float64)
        c_loss, c_grad = ce_truth(logits, target, mask, shift, torch.float32)
        e_loss = abs(c_loss.double().item() - t_loss.item()) / abs(t_loss.item())
        b_loss, b_grad = 4 * e_loss + floor, 4 * relerr(c_grad[:, :logits.shape[1] - shift], t_grad[:, :logits.shape[1] - shift]) + floor
        B, T, _ = logits.shape
        runs = []
        rows = torch.nn.functional.pad(logits, (0, pitch - K)).reshape(B, 1, T, pitch).cuda().requires_grad_(True)
        for tname, tgt in (("i32", target.int().cuda()), ("i64", target.cuda().unsqueeze(-1))):   # NHWC rows, int32 (B, T) and int64 (B, T, 1) targets
            rows.grad = None
            loss = masked_cross_entropy(rows, tgt, mask.cuda(), shift=shift, num_classes=K)
            loss.backward()
            assert torch.count_nonzero(rows.grad[..., K:]).item() == 0                  # padding columns: exactly 0
            runs.append(("nhwc." + tname, loss, rows.grad[:, 0, :, :K].clone()))
        if pitch == K:
            crit = MaskedCrossEntropyLoss()
            for name, view in (("bkt", lambda t: t), ("bkt1", lambda t: t.unsqueeze(-1))):
                x = logits.transpose(1, 2).contiguous().cuda().requires_grad_(True)      # (B, K, T)
                loss = crit(view(x), target.cuda().unsqueeze(-1), mask=mask.cuda().unsqueeze(-1), shift=shift)
                loss.backward()
                runs.append((name, loss, x.grad.transpose(1, 2)))
            # the reference's own convention on sliced tensors: the same rows, so the same loss
            xs = logits.transpose(1, 2).contiguous().cuda()
            l3 = crit(xs[:, :, :T - shift].unsqueeze(-1), target.cuda()[:, shift:].unsqueeze(-1), mask=mask.cuda().unsqueeze(-1))
            assert abs(l3.item() - runs[0][1].item()) <= 2.0 ** -22 * abs(l3.item())
        for name, loss, grad in runs:
            assert torch.isfinite(loss).item() and torch.isfinite(grad).all().item()
            assert torch.count_nonzero(grad[:, T - shift:]).item() == 0                  # the rows without a target: zero gradient
            g_loss = abs(loss.double().item() - t_loss.item()) / abs(t_loss.item())
            g_grad = relerr(grad[:, :T - shift], t_grad[:, :T - shift])
            print("K %d pitch %d shift %d %-8s loss err %.3g (bound %.3g)  grad err %.3g (bound %.3g)" % (K, pitch, shift, name, g_loss, b_loss, g_grad, b_grad))
            key = "K%d.shift%d.%s" % (K, shift, name)
            pairs[key] = {"loss_err": g_loss, "loss_bound": b_loss, "grad_err": g_grad, "grad_bound": b_grad}
    record_parity("masked_ce", pairs)
    for key, p in pairs.items():
        assert p["loss_err"] <= p["loss_bound"], (key, p)
        assert p["grad_err"] <= p["grad_bound"], (key, p)


def test_mask_equal_to_lengths():
    """1b. lengths= against mask= on a mask that IS a sequence mask: the same bits"""
    from viai_amd.wavenet import MaskedCrossEntropyLoss
    B, T, K = 3, 40, 256
    x = O.cf_uniform("cel.x", (B, K, T), -4, 4).cuda()
    target = (O.cf_uniform("cel.t", (B, T, 1), 0, 1) * K).long().clamp(max=K - 1).cuda()
    lengths = torch.tensor([T - 1, T - 15, 8]).cuda()
    mask = (torch.arange(T - 1).unsqueeze(0).cuda() < lengths.unsqueeze(1)).float().unsqueeze(-1)
    crit = MaskedCrossEntropyLoss()
    a = crit(x, target, lengths=lengths, max_len=T - 1, shift=1)
    b = crit(x, target, mask=mask, shift=1)
    c = crit(x, target, lengths=lengths, shift=1)                                       # max_len left out: the mask's missing tail is 0
    assert a.item() == b.item() == c.item()
    with pytest.raises(RuntimeError, match="Should provide either lengths or mask"):
        crit(x, target)


def test_out_of_range_targets():
    """2. a target outside [0, K) is never used as an address: on a masked-out row the loss is the in-range result, on an unmasked row NaN"""
    from viai_amd.wavenet import masked_cross_entropy
    B, T, K = 2, 24, 256
    rows = O.cf_uniform("oor.x", (B, 1, T, K), -3, 3).cuda().requires_grad_(True)
    target = (O.cf_uniform("oor.t", (B, T), 0, 1) * K).long().clamp(max=K - 1).cuda()
    mask = torch.ones(B, T).cuda()
    mask[1, 10:] = 0
    good = masked_cross_entropy(rows, target, mask)
    good.backward()
    g_good = rows.grad.clone()
    for bad_value in (K, -1, 1 << 30, -(1 << 31)):
        bad = target.clone()
        bad[1, 12], bad[1, 20] = bad_value, bad_value
        rows.grad = None
        loss = masked_cross_entropy(rows, bad, mask)
        loss.backward()
        assert loss.item() == good.item() and bits_equal(rows.grad, g_good), bad_value
        bad[0, 3] = bad_value                                                            # an unmasked row
        assert torch.isnan(masked_cross_entropy(rows.detach(), bad, mask)).item(), bad_value


def test_class_form_forward_is_a_row_gather():
    """3. the first layer on class indices equals w_eff[:, k].T + b bit for bit, w_eff from normed_weight; a class outside [0, K) gives NaN"""
    from viai_amd.wavenet import _ClassEmbed, normed_weight
    net = build()
    B, T, K = 2, 64, 256
    idx = (O.cf_uniform("ce3.idx", (B, T), 0, 1) * K).long().clamp(max=K - 1).cuda()
    with torch.no_grad():
        w = normed_weight(net.first_conv).reshape(net.first_conv.out_channels, K)
        h = _ClassEmbed.apply(idx.int(), w, net.first_conv.bias)
        want = w.t()[idx] + net.first_conv.bias                                          # (B, T, C): one fp32 addition per element, as in the kernel
        assert tuple(h.shape) == (B, 1, T, w.shape[0]) and bits_equal(h[:, 0], want)
        bad = idx.int().clone()
        bad[0, 0], bad[1, 5] = K, -1
        hb = _ClassEmbed.apply(bad, w, net.first_conv.bias)
        assert torch.isnan(hb[0, 0, 0]).all().item() and torch.isnan(hb[1, 0, 5]).all().item()
        bad[0, 0], bad[1, 5] = idx[0, 0], idx[1, 5]
        assert bits_equal(_ClassEmbed.apply(bad, w, net.first_conv.bias), h)


def test_class_form_backward_matches_dense_and_repeats_bitwise():
    """4. first_conv's weight_v / weight_g / bias gradients through the class form against the dense one-hot path (2e-3, the gradient tolerance
    of tests/test_wavenet_gpu.py); two backward runs give the same bits.  Then the layer alone at the reference's width over several row
    segments, uniform and heavily skewed classes, against an fp64 index_add."""
    from viai_amd.wavenet import MaskedCrossEntropyLoss, _ClassEmbed
    cfg = W.WNConfigOneHot
    net = build()
    B, T, K = 2, 64, cfg.out_channels
    idx = (O.cf_uniform("ce4.idx", (B, T), 0, 1) * K).long().clamp(max=K - 1).cuda()
    c = O.cf_uniform("ce4.c", (B, cfg.cin_channels, T // 16), 0, 1).cuda()
    lengths = torch.tensor([T - 1, T - 15]).cuda()
    crit = MaskedCrossEntropyLoss()
    names = ("first_conv.weight_v", "first_conv.weight_g", "first_conv.bias")
    params = dict(net.named_parameters())

    def grads(x):
        net.zero_grad(set_to_none=True)
        crit(net.forward_nhwc(x, c), idx, lengths=lengths, max_len=T - 1, shift=1).backward()
        return [params[n].grad.clone() for n in names]
    g_class, g_again = grads(idx), grads(idx)
    g_dense = grads(torch.nn.functional.one_hot(idx, K).float().transpose(1, 2).contiguous())
    for n, a, b, d in zip(names, g_class, g_again, g_dense):
        assert bits_equal(a, b), n
        assert relerr(a, d) < 2e-3, (n, relerr(a, d))
    Cc = 512
    w = O.cf_uniform("ce4.w", (Cc, K), -1, 1).cuda().requires_grad_(True)
    bias = O.cf_uniform("ce4.b", (Cc,), -1, 1).cuda().requires_grad_(True)
    for name, Bn, Tn, skew in (("uniform", 2, 2500, False), ("skewed", 3, 2100, True)):
        u = O.cf_uniform("ce4.k." + name, (Bn, Tn), 0, 1)
        k = (u * K).long().clamp(max=K - 1)
        if skew:
            k = torch.where(u < 0.9, torch.full_like(k, 127), k)                          # nine rows in ten in one class: lists longer than a chunk's quarter
        dh = O.cf_uniform("ce4.dh." + name, (Bn, 1, Tn, Cc), -1, 1).cuda()
        outs = []
        for _ in range(2):
            w.grad = bias.grad = None
            _ClassEmbed.apply(k.int().cuda(), w, bias).backward(dh)
            outs.append((w.grad.clone(), bias.grad.clone()))
        assert bits_equal(outs[0][0], outs[1][0]) and bits_equal(outs[0][1], outs[1][1]), name
        d64 = dh.double().cpu().reshape(-1, Cc)
        want = torch.zeros(K, Cc, dtype=torch.float64).index_add_(0, k.reshape(-1), d64).t()
        e_w, e_b = relerr(outs[0][0], want), relerr(outs[0][1], d64.sum(0))
        print("class_embed_bwd %s: rows %d dW err %.3g db err %.3g" % (name, Bn * Tn, e_w, e_b))
        assert e_w < 2e-3 and e_b < 2e-3, (name, e_w, e_b)
        assert torch.count_nonzero(outs[0][0][:, torch.bincount(k.reshape(-1), minlength=K) == 0]).item() == 0   # unused classes: exactly 0


def small_inputs(gold):
    cfg = W.WNConfigOneHot
    B, T, K = [int(v) for v in gold["small.meta"]]
    idx = torch.from_numpy(gold["small.idx"])
    c = O.cf_uniform("wnot.small.c", (B, cfg.cin_channels, T // 16), 0, 1)
    return B, T, K, idx.cuda(), c.cuda(), torch.from_numpy(gold["small.lengths"]).cuda()


@pytest.mark.parametrize("form", ["classes", "dense"])
def test_small_fixture_end_to_end(form, golden_dir):
    """5. the reference's training step on the small network through both input forms: yhat 1e-4, loss 1e-4 relative, the five gradients 2e-3
    (the tolerances of test_one_hot_input_wavenet_matches_reference_golden).  The class form runs the new path end to end (class gather,
    NHWC rows, shift = 1); the dense form is the reference's call, sliced tensors and all."""
    from viai_amd.wavenet import MaskedCrossEntropyLoss
    gold = np.load(golden_dir + "/wavenet_onehot_train.npz")
    B, T, K, idx, c, lengths = small_inputs(gold)
    net = build()
    crit = MaskedCrossEntropyLoss()
    if form == "classes":
        rows = net.forward_nhwc(idx, c)
        yh = rows[..., :K].squeeze(1).transpose(1, 2)
        assert bits_equal(net(idx, c), yh)                                               # forward() takes the class form too
        loss = crit(rows, idx.unsqueeze(-1), lengths=lengths, max_len=T - 1, shift=1)
    else:
        x = torch.nn.functional.one_hot(idx, K).float().transpose(1, 2).contiguous()
        yh = net(x, c)
        loss = crit(yh[:, :, :-1].unsqueeze(-1), idx.unsqueeze(-1)[:, 1:], lengths=lengths, max_len=T - 1)
    assert tuple(yh.shape) == (B, K, T)
    assert relerr(yh, gold["small.yhat"]) < 1e-4
    assert abs(loss.item() - float(gold["small.loss"])) < 1e-4 * float(gold["small.loss"])
    loss.backward()
    params = dict(net.named_parameters())
    keys = [k for k in gold.files if k.startswith("small.g.")]
    assert len(keys) == 5
    for k in keys:
        assert relerr(params[k[len("small.g."):]].grad, gold[k]) < 2e-3, k


def test_reference_width_fixture(golden_dir):
    """6. 24 layers / 512 / 512 / 256, K = 256, B = 1, T = 1024 from class indices: loss 1e-4 relative, gradient digests by the rule of
    test_reference_size_wavenet_matches_reference_digests (2e-3 on the norm entry, 4e-3 on the sampled entries)."""
    from viai_amd.wavenet import masked_cross_entropy, sequence_mask
    gold = np.load(golden_dir + "/wavenet_onehot_train.npz")
    cfg = WNConfigOneHotFull
    B, T, K = [int(v) for v in gold["full.meta"]]
    idx = (O.cf_uniform("wnot.full.idx", (B, T), 0, 1) * K).long().clamp(max=K - 1).cuda()
    c = O.cf_uniform("wnot.full.c", (B, cfg.cin_channels, T // 256), 0, 1).cuda()
    lengths = torch.from_numpy(gold["full.lengths"]).cuda()
    net = build(cfg, "WNOF.")
    rows = net.forward_nhwc(idx, c)
    assert tuple(rows.shape) == (B, 1, T, K)
    yh = rows.squeeze(1).transpose(1, 2).contiguous()
    assert relerr(O.digest(yh, 256), gold["full.yhat.dg"]) < 1e-4
    loss = masked_cross_entropy(rows, idx, sequence_mask(lengths, T - 1), shift=1)
    assert abs(loss.item() - float(gold["full.loss"])) < 1e-4 * float(gold["full.loss"])
    loss.backward()
    params = dict(net.named_parameters())
    keys = [k for k in gold.files if k.startswith("full.g.")]
    assert len(keys) == 11
    for k in keys:
        dg, ref = O.digest(params[k[len("full.g."):-3]].grad), gold[k]
        assert abs(dg[2] - ref[2]) < 2e-3 * ref[2], (k, dg[2], ref[2])
        assert np.linalg.norm(dg[3:] - ref[3:]) < 4e-3 * np.linalg.norm(ref[3:]), k


def test_mulaw_quantize():
    """7. the expected classes on the mid-interval check vectors, exactly; decode(quantize(x)) within one quantisation bin of x"""
    from viai_amd.wavenet import mulaw_decode, mulaw_quantize
    x, want = mulaw_vectors()
    got = mulaw_quantize(torch.from_numpy(x).float().cuda())
    assert got.dtype == torch.int64 and torch.equal(got.cpu(), torch.from_numpy(want))
    assert mulaw_quantize(torch.tensor([-1.5, 1.5, 2.0]).cuda()).tolist() == [0, 255, 255]      # the clamp
    u = O.cf_uniform("mq.u", (4096,), -1, 1)
    k = mulaw_quantize(u.cuda().reshape(64, 64))
    assert tuple(k.shape) == (64, 64) and int(k.min()) >= 0 and int(k.max()) <= 255
    back = mulaw_decode(k).cpu().reshape(-1).double()
    edges = mulaw_decode(torch.arange(256).cuda()).cpu().double()                        # class k covers [edge k, edge k + 1)
    kk = k.cpu().reshape(-1)
    hi = (kk + 1).clamp(max=255)
    width = edges[hi] - edges[hi - 1]                                                    # the bin of class k (the last bin for k = 255)
    assert bool(((back - u.double()).abs() <= width + 1e-6).all())
    y64 = torch.sign(u.double()) * torch.log1p(255 * u.double().abs()) / np.log1p(255.0)
    k64 = ((y64 + 1) / 2 * 255).floor().long().clamp(0, 255)
    assert int((kk - k64).abs().max()) <= 1 and float((kk != k64).float().mean()) < 1e-3    # off only where fp32 rounds across an edge


def test_dense_float_input_keeps_its_path(monkeypatch):
    """8. forward() with a float (B, K, T) tensor still runs conv1d_apply on the first layer: the tensor that layer produces inside forward()
    is bit for bit the one conv1d_apply gives when called directly, and the class form is not touched."""
    from viai_amd import wavenet as wn
    cfg = W.WNConfigOneHot
    net = build().eval()
    B, T, K = 2, 64, cfg.out_channels
    idx = (O.cf_uniform("ce8.idx", (B, T), 0, 1) * K).long().clamp(max=K - 1).cuda()
    x = torch.nn.functional.one_hot(idx, K).float().transpose(1, 2).contiguous()
    c = O.cf_uniform("ce8.c", (B, cfg.cin_channels, T // 16), 0, 1).cuda()
    seen, real = [], wn.conv1d_apply

    def spy(xx, m, *a, **k):
        out = real(xx, m, *a, **k)
        if m is net.first_conv:
            seen.append(out)
        return out

    def never(*a, **k):
        raise AssertionError("the class form ran on float input")
    monkeypatch.setattr(wn, "conv1d_apply", spy)
    monkeypatch.setattr(wn._ClassEmbed, "apply", never)
    with torch.no_grad():
        y = net(x, c)
        direct = real(x.transpose(1, 2).unsqueeze(1).contiguous(), net.first_conv)
    assert len(seen) == 1 and bits_equal(seen[0], direct)
    monkeypatch.undo()
    with torch.no_grad():
        assert relerr(net(idx, c), y) < 1e-4                                             # and the class form computes the same network
