#!/usr/bin/env python
"""Generate tests/golden/*.npz from the REFERENCE's own modules (build container only).

Imports `MelEncoder`, `MelDecoder`, `MelDiscriminator` and `GANLoss` from
/root/reference (read-only; nothing is copied) behind the stub config modules
in tools/oracle_stubs/ (SURVEY.md §8c recipe), loads the closed-form weights of
oracle/viai_oracle.py into them, runs the declared pix2pix-ordered G+D step
 with torch autograd + torch.optim.Adam, and

  1. asserts the oracle restatement reproduces every captured quantity, and
  2. writes the reference's outputs as small fixtures under tests/golden/.

The fixtures are data (inputs are regenerated from the closed-form generator;
expected outputs are stored), never reference source text.

Run:  python tools/make_goldens.py            (needs /root/reference)
"""
import os
import sys
import types
from collections import OrderedDict

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(ROOT, "tools", "oracle_stubs"))
sys.path.insert(0, REF)
sys.path.insert(0, ROOT)
for name in ("cv2", "Data_loaders.mel_loader", "Data_loaders.AV_loader"):
    sys.modules.setdefault(name, types.ModuleType(name))
import Data_loaders  # noqa: E402  (reference package; empty __init__)
Data_loaders.mel_loader = sys.modules["Data_loaders.mel_loader"]
Data_loaders.AV_loader = sys.modules["Data_loaders.AV_loader"]

from networks import Inpainting_Networks as RefEnc          # noqa: E402
from networks import New_Inpainting_Networks as RefDec      # noqa: E402
from networks import Discriminator_Networks as RefDis       # noqa: E402
import loss_functions as RefLoss                            # noqa: E402

from oracle import viai_oracle as O                         # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
LAMBDA_L1 = O.StepConfig.lambda_l1


def load_into(module, sd):
    missing, unexpected = module.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    return module


def ref_models(F_bins):
    RefEnc.hparams.cin_channels = F_bins
    E = load_into(RefEnc.MelEncoder(), O.encoder_state())
    G = load_into(RefDec.MelDecoder(), O.decoder_state())
    D = load_into(RefDis.MelDiscriminator(), O.disc_state())
    E.hparams.cin_channels = F_bins
    return E, G, D


BN_SHADOWED_BIAS = ("deconv1_1.bias", "deconv1_2.bias", "conv6_1.bias")   # bias in front of BN: true grad is 0


def ref_step(E, G, D, optG, optD, gan, s, mask, update=True):
    """The declared step with the reference's modules.
    update=False skips the two optimizer steps (the well-conditioned parity
    target, see oracle.step_no_update)."""
    cap = {}
    s_in = s * mask
    feats = E(s_in.view(s.size(0), s.size(2), s.size(3)))
    fake = G(feats, s.size())
    fake.retain_grad()
    # D step
    for p in D.parameters():
        p.requires_grad_(True)
    optD.zero_grad()
    pred_real = D(s)                                   # declared order: real first, then fake (BN running statistics)
    pred_fake_d = D(fake.detach())
    loss_d = 0.5 * (gan(pred_fake_d, False) + gan(pred_real, True))
    loss_d.backward()
    cap["grads_D"] = {k: p.grad.clone() for k, p in D.named_parameters()}
    if update:
        optD.step()
    # G step
    for p in D.parameters():
        p.requires_grad_(False)
    optG.zero_grad()
    pred_fake_g = D(fake)
    loss_g_gan = gan(pred_fake_g, True)
    loss_l1 = torch.nn.functional.l1_loss(fake, s)
    loss_g = loss_g_gan + LAMBDA_L1 * loss_l1
    loss_g.backward()
    cap["grads_E"] = {k: (p.grad.clone() if p.grad is not None else None) for k, p in E.named_parameters()}
    cap["grads_G"] = {k: (p.grad.clone() if p.grad is not None else None) for k, p in G.named_parameters()}
    if update:
        optG.step()
    cap.update(fake=fake.detach(), feats=[f.detach() for f in feats], pred_fake_d=pred_fake_d.detach(),
               pred_real=pred_real.detach(), pred_fake_g=pred_fake_g.detach(), loss_d=loss_d.detach(),
               loss_g=loss_g.detach(), loss_g_gan=loss_g_gan.detach(), loss_l1=loss_l1.detach(),
               d_fake=fake.grad.detach().clone())
    return cap


def relerr(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def fresh(F_bins):
    E, G, D = ref_models(F_bins)
    E.train(); G.train(); D.train()
    gan = RefLoss.GANLoss(use_lsgan=False, device=torch.device("cpu"))
    c = O.StepConfig
    optG = torch.optim.Adam(list(E.parameters()) + list(G.parameters()), lr=c.lr, betas=(c.beta1, c.beta2), eps=c.eps)
    optD = torch.optim.Adam(D.parameters(), lr=c.lr, betas=(c.beta1, c.beta2), eps=c.eps)
    return E, G, D, optG, optD, gan


def run_case(name, B, F_bins, T, steps, full):
    torch.manual_seed(0)
    s = O.cf_uniform("s.%s" % name, (B, 1, F_bins, T))
    mask = O.make_mask(B, T, "mask.%s" % name)
    out = OrderedDict()
    out["meta"] = np.array([B, F_bins, T, steps], dtype=np.int64)
    worst = 0.0

    # ---------------- (1) no-update step: the well-conditioned parity target
    E, G, D, optG, optD, gan = fresh(F_bins)
    cap = ref_step(E, G, D, optG, optD, gan, s, mask, update=False)
    oE, oG, oD = O.encoder_state(), O.decoder_state(), O.disc_state()
    ocap = O.step_no_update(oE, oG, oD, s, mask)
    for k in ("fake", "pred_fake_d", "pred_real", "pred_fake_g", "d_fake", "loss_d", "loss_g", "loss_l1"):
        e = relerr(ocap[k], cap[k]); worst = max(worst, e)
        assert e < (1e-3 if k == "d_fake" else 5e-5), (name, k, e)
    for i, (fo, fr) in enumerate(zip(ocap["feats"], cap["feats"])):
        e = relerr(fo, fr); worst = max(worst, e)
        assert e < 5e-5, (name, "feat", i, e)
    for grp in ("grads_D", "grads_E", "grads_G"):
        for k, g in cap[grp].items():
            og = ocap[grp][k]
            if g is None:
                assert og is None, (grp, k)
                continue
            if grp == "grads_G" and k in BN_SHADOWED_BIAS:
                assert g.abs().max() < 1e-4 and og.abs().max() < 1e-4
                continue
            e = relerr(og, g); worst = max(worst, e)
            # two torch-CPU fp32 evaluations of the same gradient differ by the conditioning of the backward chain, which
            # grows with the reduction sizes: 3e-3 at cfg 1, 5e-3 at the benchmark size (see tests/test_networks_gpu.py)
            assert e < (2e-2 if name == "cfg2" else 5e-3), (name, grp, k, e)
    for mod, osd, nm in ((E, oE, "E"), (G, oG, "G"), (D, oD, "D")):
        for k, v in mod.state_dict().items():
            if O.is_buffer(k):
                if "num_batches" in k:
                    assert int(v) == int(osd[k]), (nm, k)
                else:
                    e = relerr(osd[k], v); worst = max(worst, e)
                    assert e < 1e-4, (name, nm, k, e)
                out["nu.state." + nm + "." + k] = v.numpy().copy()
    if full:
        for k in ("fake", "pred_fake_d", "pred_real", "pred_fake_g", "d_fake"):
            out["nu." + k] = cap[k].numpy()
        for i, f in enumerate(cap["feats"]):
            out["nu.feat%d" % i] = f.numpy()
    else:
        for k in ("fake", "pred_fake_d", "pred_real", "pred_fake_g", "d_fake"):
            out["nu." + k + ".dg"] = O.digest(cap[k])
        for i, f in enumerate(cap["feats"]):
            out["nu.feat%d.dg" % i] = O.digest(f)
    for k in ("loss_d", "loss_g", "loss_g_gan", "loss_l1"):
        out["nu." + k] = np.float64(cap[k].item())
    for grp in ("grads_D", "grads_E", "grads_G"):
        for k, g in cap[grp].items():
            if g is not None:
                out["nu." + grp + "." + k + ".dg"] = O.digest(g)

    # ---------------- (2) chained steps with Adam: losses only, loose (sign-flip chaos)
    E, G, D, optG, optD, gan = fresh(F_bins)
    oE, oG, oD = O.encoder_state(), O.decoder_state(), O.disc_state()
    ooG, ooD = O.new_optimizers(oE, oG, oD)
    for it in range(steps):
        cap = ref_step(E, G, D, optG, optD, gan, s, mask, update=True)
        ocap = O.train_step(oE, oG, oD, ooG, ooD, s, mask)
        for k in ("loss_d", "loss_g", "loss_l1"):
            e = relerr(ocap[k], cap[k])
            assert e < 3e-2, (name, it, k, e)
            out["ch.step%d.%s" % (it, k)] = np.float64(cap[k].item())
    path = os.path.join(OUT, "step_%s.npz" % name)
    np.savez_compressed(path, **out)
    print("%-10s B=%d F=%d T=%d steps=%d  worst oracle-vs-reference rel err (no-update) %.2e  -> %s (%.1f KB)"
          % (name, B, F_bins, T, steps, worst, os.path.relpath(path, ROOT), os.path.getsize(path) / 1024))


def ganloss_soft_goldens():
    """GANLoss(softlabel=True) (loss_functions.py:90-99): the label is real - U(0, 0.1) / fake + U(0, 0.1) from Python's `random`; with
    the generator seeded the reference's values are reproducible -- and so is the ORDER of its draws (one per call)."""
    import random
    p = O.cf_uniform("gl.p", (4, 1, 8, 4), 0.01, 0.99)
    out = OrderedDict()
    for lsgan in (False, True):
        crit = RefLoss.GANLoss(use_lsgan=lsgan, device=torch.device("cpu"))
        random.seed(20260929)
        vals = [crit(p, real, softlabel=True).item() for real in (True, False, True, True, False)]
        out["lsgan%d" % int(lsgan)] = np.array(vals, dtype=np.float64)
    path = os.path.join(OUT, "ganloss_soft.npz")
    np.savez_compressed(path, **out)
    print("ganloss_soft -> %s (%.1f KB)" % (os.path.relpath(path, ROOT), os.path.getsize(path) / 1024))


CHAIN_STEPS = 3
SHADOWED_CHAIN = ("G.deconv1_1.bias", "G.deconv1_2.bias", "G.conv6_1.bias")   # bias in front of train-mode BN: exact gradient 0


def chain_goldens():
    """"params after 1 and 3 Adam steps".  The declared step run three times with the REFERENCE's modules +
    torch.optim.Adam on the tie-free tiny input (oracle.separated_input); after every step 256 strided samples of EVERY parameter
    tensor of E, G and D (and every BatchNorm running statistic) are stored, plus how far the oracle's own chain (second torch-CPU fp32
    implementation of the same arithmetic) is from the reference's at that step -- the noise floor any third implementation is
    judged against.  Adam's update is lr * m / sqrt(v): where a gradient is at the rounding-noise level, or changes sign between
    steps, two correct fp32 implementations move that weight in different directions; the relative PARAMETER error that follows is
    ~2e-4 after one step and grows past 1e-3 by the third (printed below)."""
    B, F_bins, T = 2, 80, 32
    s = O.cf_uniform("s.tiny", (B, 1, F_bins, T))
    mask = O.make_mask(B, T, "mask.tiny")
    s2 = O.separated_input(s, mask)
    E, G, D, optG, optD, gan = fresh(F_bins)
    oE, oG, oD = O.encoder_state(), O.decoder_state(), O.disc_state()
    ooG, ooD = O.new_optimizers(oE, oG, oD)
    out = OrderedDict()
    out["meta"] = np.array([B, F_bins, T, CHAIN_STEPS], dtype=np.int64)
    for it in range(CHAIN_STEPS):
        cap = ref_step(E, G, D, optG, optD, gan, s2, mask, update=True)
        ocap = O.train_step(oE, oG, oD, ooG, ooD, s2, mask)
        for k in ("loss_d", "loss_g", "loss_l1"):
            out["step%d.%s" % (it + 1, k)] = np.float64(cap[k].item())
        floor = []
        for nm, mod, osd in (("E", E, oE), ("G", G, oG), ("D", D, oD)):
            num = den = 0.0
            for k, v in mod.state_dict().items():
                if "num_batches" in k:
                    continue
                out["step%d.%s.%s" % (it + 1, nm, k)] = O.strided_samples(v)
                if not O.is_buffer(k) and (nm + "." + k) not in SHADOWED_CHAIN:
                    num += (v.double() - osd[k].double()).pow(2).sum().item()
                    den += v.double().pow(2).sum().item()
            floor.append((num / den) ** 0.5)
        out["step%d.oracle_vs_reference" % (it + 1)] = np.array(floor)
        print("chain step %d: oracle-vs-reference relative parameter error  E %.2e  G %.2e  D %.2e   (loss_d %.5f loss_g %.4f)"
              % (it + 1, floor[0], floor[1], floor[2], cap["loss_d"].item(), cap["loss_g"].item()))
        assert max(floor) < (1e-3 if it == 0 else 1e-2), floor
    path = os.path.join(OUT, "step_chain.npz")
    np.savez_compressed(path, **out)
    print("chain -> %s (%.1f KB)" % (os.path.relpath(path, ROOT), os.path.getsize(path) / 1024))


def av_goldens():
    """AV decoders + sync / domain discriminators at the native MUSICES shape (80 x 208; SURVEY.md §8a:
    MelDecoderImage needs bottleneck h == 1, Inpainting_Dis needs F/8 == 10, DomainDis needs T/16 == 13)."""
    out = OrderedDict()
    B, F_bins, T = 2, 80, 208
    s = O.cf_uniform("av.s", (B, 1, F_bins, T))
    video = O.cf_uniform("av.video", (B, 256, 1, 13), -1, 1)
    fea = O.cf_uniform("av.fea", (B, 512, 52), -1, 1)
    RefEnc.hparams.cin_channels = F_bins
    E = load_into(RefEnc.MelEncoder(), O.encoder_state()); E.hparams.cin_channels = F_bins; E.train()
    feats = [f.detach() for f in E(s.view(B, F_bins, T))]
    ofeats = [f.detach() for f in O.encoder_forward(O.encoder_state(), s.view(B, F_bins, T))]
    for variant, cls in (("image", RefDec.MelDecoderImage), ("image2", RefDec.MelDecoderImage2), ("old", RefDec.MelDecoder_old)):
        G = load_into(cls(), O.decoder_variant_state(variant)); G.train()
        args = (feats, s.size(), video) if variant != "old" else (feats, s.size())
        fake = G(*args)
        fake.mean().backward()
        osd = O._leafify(O.decoder_variant_state(variant))
        ofake = O.decoder_variant_forward(osd, variant, ofeats, s.shape, video if variant != "old" else None)
        assert relerr(ofake, fake) < 5e-5, (variant, relerr(ofake, fake))
        key = "deconv1_1_1.weight" if variant != "old" else "deconv1_1.weight"
        (og,) = torch.autograd.grad(ofake.mean(), osd[key])
        assert relerr(og, dict(G.named_parameters())[key].grad) < 2e-2, (variant, relerr(og, dict(G.named_parameters())[key].grad))
        out["dec_%s.fake" % variant] = fake.detach().numpy()
        out["dec_%s.g.%s.dg" % (variant, key)] = O.digest(dict(G.named_parameters())[key].grad)
        out["dec_%s.g.conv6_2.weight.dg" % variant] = O.digest(G.conv6_2.weight.grad)
    # init_deconv_1_1_1
    G = RefDec.MelDecoderImage(); G.init_deconv_1_1_1()
    assert torch.equal(G.deconv1_1_1.weight[:256], G.deconv1_1.weight) and torch.equal(G.deconv1_1_1.weight[256:], G.deconv1_1.weight)
    # Inpainting_Dis
    ID = load_into(RefDis.Inpainting_Dis(), O.inpainting_dis_state()); ID.train()
    y = ID(s, fea)
    y.mean().backward()
    osd = O._leafify(O.inpainting_dis_state())
    oy = O.inpainting_dis_forward(osd, s, fea)
    assert tuple(y.shape) == (B, 21) and relerr(oy, y) < 5e-5, relerr(oy, y)
    (og,) = torch.autograd.grad(oy.mean(), osd["mel_conv2.weight"])
    assert relerr(og, ID.mel_conv2.weight.grad) < 5e-3
    out["inp_dis.out"] = y.detach().numpy()
    for k in ("mel_conv1.weight", "mel_conv4.weight", "vid_conv1.weight", "conv.weight", "vid_bn1.weight"):
        out["inp_dis.g.%s.dg" % k] = O.digest(dict(ID.named_parameters())[k].grad)
    # DomainDis
    RefDis.hparams.length_feature = 256
    DD = load_into(RefDis.DomainDis(), O.domain_dis_state())
    emb = O.cf_uniform("av.emb", (4, 256, 1, 13), -1, 1)
    y = DD(emb)
    y.mean().backward()
    osd = O._leafify(O.domain_dis_state())
    oy = O.domain_dis_forward(osd, emb)
    assert tuple(y.shape) == (4, 1) and relerr(oy, y) < 5e-6
    out["dom_dis.out"] = y.detach().numpy()
    for k in ("conv1.weight", "fc1.weight", "fc1.bias", "fc2.weight"):
        out["dom_dis.g.%s.dg" % k] = O.digest(dict(DD.named_parameters())[k].grad)
    path = os.path.join(OUT, "av.npz")
    np.savez_compressed(path, **out)
    print("av -> %s (%.1f KB)" % (os.path.relpath(path, ROOT), os.path.getsize(path) / 1024))


def resnet_goldens():
    """ImageEmbedding2 (two ResNet-18s + temporal convs) on 4 frames of 224x224 (B=1, N=4)."""
    from networks import Image_Embedding as RefIE
    out = OrderedDict()
    video = O.cf_uniform("ie.video", (1, 4, 3, 224, 224), -1, 1)
    flow = O.cf_uniform("ie.flow", (1, 4, 2, 224, 224), -1, 1)
    M = load_into(RefIE.ImageEmbedding2(), O.image_embedding2_state()); M.train()
    o, fea = M(video, flow)
    (o.pow(2).mean() + fea.pow(2).mean()).backward()
    osd = O._leafify(O.image_embedding2_state())
    oo, ofea = O.image_embedding2_forward(osd, video, flow)
    assert tuple(o.shape) == (1, 256, 1, 1) and tuple(fea.shape) == (1, 512, 4)
    assert relerr(ofea, fea) < 5e-5 and relerr(oo, o) < 5e-5, (relerr(ofea, fea), relerr(oo, o))
    keys = ("image_single_model.conv1.weight", "flow_single_model.conv1.weight", "image_single_model.layer2.0.downsample.0.weight",
            "image_single_model.layer4.1.conv2.weight", "image_single_model.fc.weight", "flow_single_model.layer1.0.bn1.weight", "conv_1.weight", "conv_2.weight")
    og = torch.autograd.grad(oo.pow(2).mean() + ofea.pow(2).mean(), [osd[k] for k in keys])
    for k, g in zip(keys, og):
        e = relerr(g, dict(M.named_parameters())[k].grad)
        assert e < 2e-2, (k, e)
        out["g.%s.dg" % k] = O.digest(dict(M.named_parameters())[k].grad)
    assert M.bn_1.weight.grad is None
    out["out"] = o.detach().numpy(); out["fea_cat"] = fea.detach().numpy()
    out["rm.image.bn1"] = M.image_single_model.bn1.running_mean.numpy().copy()
    out["rv.flow.layer3.0.downsample.1"] = M.flow_single_model.layer3[0].downsample[1].running_var.numpy().copy()
    # ImageEmbedding: bn_1 is dead except for its running statistics
    M1 = load_into(RefIE.ImageEmbedding(), O.image_embedding2_state()); M1.train()
    o1 = M1(video, flow)
    sd1 = O.image_embedding2_state()
    oo1, _ = O.image_embedding2_forward(sd1, video, flow, dead_bn=True)
    assert relerr(oo1, o1) < 5e-5 and relerr(sd1["bn_1.running_var"], M1.bn_1.running_var) < 1e-4
    out["ie1.out"] = o1.detach().numpy(); out["ie1.bn_1.running_var"] = M1.bn_1.running_var.numpy().copy()
    path = os.path.join(OUT, "resnet.npz")
    np.savez_compressed(path, **out)
    print("resnet -> %s (%.1f KB)" % (os.path.relpath(path, ROOT), os.path.getsize(path) / 1024))


def wavenet_goldens():
    """WaveNet (small config) teacher-forced forward + MoL loss + gradients, MoL sampler, and a short
    incremental_forward run, all from the reference's wavenet_vocoder package."""
    import Config
    from oracle import wavenet_oracle as W
    cfg = W.WNConfig
    from wavenet_vocoder import wavenet as RW, mixture as RM
    net = RW.WaveNet(out_channels=cfg.out_channels, layers=cfg.layers, stacks=cfg.stacks, residual_channels=cfg.residual_channels,
                     gate_channels=cfg.gate_channels, skip_out_channels=cfg.skip_out_channels, kernel_size=cfg.kernel_size, dropout=0.0,
                     cin_channels=cfg.cin_channels, gin_channels=-1, n_speakers=None, weight_normalization=True,
                     upsample_conditional_features=True, upsample_scales=list(cfg.upsample_scales),
                     freq_axis_kernel_size=cfg.freq_axis_kernel_size, scalar_input=True)
    sd = W.wavenet_state(cfg)
    assert list(net.state_dict().keys()) == list(sd.keys()), set(net.state_dict()) ^ set(sd)
    load_into(net, sd)
    out = OrderedDict()
    B, T = 2, 64
    x = O.cf_uniform("wn.x", (B, 1, T), -1, 1)
    c = O.cf_uniform("wn.c", (B, cfg.cin_channels, T // 16), 0, 1)
    y = O.cf_uniform("wn.y", (B, T, 1), -1, 1)
    y[0, 3, 0], y[1, 5, 0] = -1.0, 1.0                         # the two edge branches of the MoL likelihood
    mask = torch.ones(B, T, 1); mask[1, T - 10:] = 0
    net.train()
    yh = net(x, c)
    losses = RM.discretized_mix_logistic_loss(yh, y, num_classes=65536, log_scale_min=float(np.log(1e-14)), reduce=False)
    loss = (losses * mask).sum() / mask.sum()
    loss.backward()
    osd = O._leafify(sd)
    oyh = W.wavenet_forward(osd, x, c, cfg)
    assert relerr(oyh, yh) < 1e-5, relerr(oyh, yh)
    oloss = W.mol_loss(oyh, y, mask)
    assert abs(oloss.item() - loss.item()) < 1e-5 * abs(loss.item())
    keys = ("first_conv.weight_g", "first_conv.bias", "conv_layers.0.conv.weight_g", "conv_layers.3.conv.weight_v", "conv_layers.1.conv1x1c.weight_v",
            "conv_layers.2.conv1x1_skip.bias", "last_conv_layers.3.weight_v", "upsample_conv.0.weight_v", "upsample_conv.2.bias")
    og = torch.autograd.grad(oloss, [osd[k] for k in keys])
    for k, g in zip(keys, og):
        ref = dict(net.named_parameters())[k].grad
        assert relerr(g, ref) < 1e-3, (k, relerr(g, ref))
        out["g.%s" % k] = ref.numpy().copy()
    out["yhat"] = yh.detach().numpy(); out["loss"] = np.float64(loss.item()); out["loss_rows"] = losses.detach().numpy()
    # sampler with injected uniforms: patch Tensor.uniform_ so the reference draws OUR numbers
    u1 = O.cf_uniform("wn.u1", (B, T, 10), 1e-5, 1 - 1e-5)
    u2 = O.cf_uniform("wn.u2", (B, T), 1e-5, 1 - 1e-5)
    draws = [u1, u2]
    orig = torch.Tensor.uniform_
    torch.Tensor.uniform_ = lambda self, a=0, b=1: self.copy_(draws.pop(0))
    try:
        smp = RM.sample_from_discretized_mix_logistic(yh.detach(), log_scale_min=-7.0)
    finally:
        torch.Tensor.uniform_ = orig
    assert relerr(W.mol_sample(yh.detach(), u1, u2), smp) < 1e-6
    out["sample"] = smp.numpy()
    # incremental_forward, free-running for 24 steps (teacher-forced on the first 4), injected uniforms per step
    net.eval()
    Tg = 32
    cg = O.cf_uniform("wn.cg", (B, cfg.cin_channels, Tg // 16), 0, 1)
    v1 = O.cf_uniform("wn.v1", (B, Tg, 10), 1e-5, 1 - 1e-5)
    v2 = O.cf_uniform("wn.v2", (B, Tg), 1e-5, 1 - 1e-5)
    tin = O.cf_uniform("wn.tin", (B, 1, 4), -1, 1)
    seq = []
    for t in range(Tg):
        seq += [v1[:, t:t + 1, :].reshape(B, 1, 10), v2[:, t:t + 1].reshape(B, 1)]
    torch.Tensor.uniform_ = lambda self, a=0, b=1: self.copy_(seq.pop(0).reshape(self.shape))
    try:
        with torch.no_grad():
            gen = net.incremental_forward(initial_input=None, c=cg, g=None, T=Tg, test_inputs=tin, tqdm=lambda z: z, softmax=False,
                                          quantize=False, log_scale_min=-7.0)
    finally:
        torch.Tensor.uniform_ = orig
    ogen = W.incremental_forward(sd, cg, Tg, v1, v2, cfg, test_inputs=tin)
    assert tuple(gen.shape) == (B, 1, Tg) and relerr(ogen, gen) < 1e-4, relerr(ogen, gen)
    out["gen"] = gen.numpy()
    path = os.path.join(OUT, "wavenet.npz")
    np.savez_compressed(path, **out)
    print("wavenet -> %s (%.1f KB)" % (os.path.relpath(path, ROOT), os.path.getsize(path) / 1024))


def wavenet_full_goldens():
    """WaveNet at the REFERENCE's size (24 layers / 4 stacks / 512 / 512 / 256, hop 256; SURVEY.md section 8c "one full-size
    digest"): teacher-forced forward, MoL loss and gradient digests at B1, T = 1024 from the reference's wavenet_vocoder."""
    import Config  # noqa: F401
    from oracle import wavenet_oracle as W
    cfg = W.WNConfigFull
    from wavenet_vocoder import wavenet as RW, mixture as RM
    net = RW.WaveNet(out_channels=cfg.out_channels, layers=cfg.layers, stacks=cfg.stacks, residual_channels=cfg.residual_channels,
                     gate_channels=cfg.gate_channels, skip_out_channels=cfg.skip_out_channels, kernel_size=cfg.kernel_size, dropout=0.0,
                     cin_channels=cfg.cin_channels, gin_channels=-1, n_speakers=None, weight_normalization=True,
                     upsample_conditional_features=True, upsample_scales=list(cfg.upsample_scales),
                     freq_axis_kernel_size=cfg.freq_axis_kernel_size, scalar_input=True)
    sd = W.wavenet_state(cfg)
    assert list(net.state_dict().keys()) == list(sd.keys())
    assert sum(p.numel() for p in net.parameters()) == 24737396           # SURVEY.md section 8a [probe]
    load_into(net, sd)
    net.train()
    B, T = 1, 1024
    x = O.cf_uniform("wnf.x", (B, 1, T), -1, 1)
    c = O.cf_uniform("wnf.c", (B, cfg.cin_channels, T // 256), 0, 1)
    y = O.cf_uniform("wnf.y", (B, T, 1), -1, 1)
    yh = net(x, c)
    losses = RM.discretized_mix_logistic_loss(yh, y, num_classes=65536, log_scale_min=float(np.log(1e-14)), reduce=False)
    loss = losses.mean()
    loss.backward()
    oyh = W.wavenet_forward(sd, x, c, cfg)
    assert relerr(oyh, yh) < 1e-5, relerr(oyh, yh)
    assert abs(W.mol_loss(oyh, y, torch.ones(B, T, 1)).item() - loss.item()) < 1e-5 * abs(loss.item())
    out = OrderedDict()
    out["meta"] = np.array([B, T], dtype=np.int64)
    out["yhat.dg"] = O.digest(yh, 256)
    out["yhat_tail"] = yh.detach()[:, :, -64:].numpy()
    out["loss"] = np.float64(loss.item())
    params = dict(net.named_parameters())
    for k in ("first_conv.weight_g", "conv_layers.0.conv.weight_v", "conv_layers.11.conv.weight_g", "conv_layers.23.conv.weight_v",
              "conv_layers.23.conv1x1c.weight_v", "conv_layers.12.conv1x1_skip.bias", "conv_layers.5.conv1x1_out.weight_v",
              "last_conv_layers.1.weight_v", "last_conv_layers.3.weight_v", "upsample_conv.0.weight_v", "upsample_conv.6.bias"):
        out["g.%s.dg" % k] = O.digest(params[k].grad)
    path = os.path.join(OUT, "wavenet_full.npz")
    np.savez_compressed(path, **out)
    print("wavenet_full -> %s (%.1f KB)" % (os.path.relpath(path, ROOT), os.path.getsize(path) / 1024))


def wavenet_deep_goldens():
    """Incremental synthesis at the REFERENCE's depth (24 layers / 4 stacks, dilations 1 .. 32; reduced width), B = 2, T = 160: every
    ring buffer of conv.py:17-46 (length (k - 1) d + 1 <= 65) wraps at least twice.  Two runs of the reference's
    `incremental_forward` (wavenet.py:237-364) with the sampler's uniforms injected: teacher-forced over the whole length (each output is a
    smooth function of that step's logits: no feedback) and free-running after four teacher-forced samples."""
    import Config  # noqa: F401
    from oracle import wavenet_oracle as W
    cfg = W.WNConfigDeep
    from wavenet_vocoder import wavenet as RW
    net = RW.WaveNet(out_channels=cfg.out_channels, layers=cfg.layers, stacks=cfg.stacks, residual_channels=cfg.residual_channels,
                     gate_channels=cfg.gate_channels, skip_out_channels=cfg.skip_out_channels, kernel_size=cfg.kernel_size, dropout=0.0,
                     cin_channels=cfg.cin_channels, gin_channels=-1, n_speakers=None, weight_normalization=True,
                     upsample_conditional_features=True, upsample_scales=list(cfg.upsample_scales),
                     freq_axis_kernel_size=cfg.freq_axis_kernel_size, scalar_input=True)
    sd = W.wavenet_state(cfg, tag="WND.")
    assert list(net.state_dict().keys()) == list(sd.keys())
    load_into(net, sd)
    net.eval()
    assert [l.conv.dilation[0] for l in net.conv_layers] == [1, 2, 4, 8, 16, 32] * 4
    B, T = 2, 160
    c = O.cf_uniform("wnd.c", (B, cfg.cin_channels, T // 16), 0, 1)
    v1 = O.cf_uniform("wnd.v1", (B, T, 10), 1e-5, 1 - 1e-5)
    v2 = O.cf_uniform("wnd.v2", (B, T), 1e-5, 1 - 1e-5)
    xin = O.cf_uniform("wnd.xin", (B, 1, T), -1, 1)
    out = OrderedDict()
    out["meta"] = np.array([B, T, cfg.layers, cfg.stacks], dtype=np.int64)
    orig = torch.Tensor.uniform_

    def run(test_inputs):
        seq = []
        for t in range(T):
            seq += [v1[:, t:t + 1, :].reshape(B, 1, 10), v2[:, t:t + 1].reshape(B, 1)]
        torch.Tensor.uniform_ = lambda self, a=0, b=1: self.copy_(seq.pop(0).reshape(self.shape))
        try:
            with torch.no_grad():
                return net.incremental_forward(initial_input=None, c=c, g=None, T=T, test_inputs=test_inputs, tqdm=lambda z: z,
                                               softmax=False, quantize=False, log_scale_min=-7.0)
        finally:
            torch.Tensor.uniform_ = orig
    gen_tf = run(xin)
    gen_free = run(xin[:, :, :4].contiguous())
    assert tuple(gen_tf.shape) == (B, 1, T) and tuple(gen_free.shape) == (B, 1, T)
    # the oracle's definition-of-causality restatement (batch forward on the teacher-forced input) reproduces the teacher-forced run
    with torch.no_grad():
        yh = W.wavenet_forward(sd, xin, c, cfg)                       # logits at t from inputs <= t
        osmp = W.mol_sample(yh, v1, v2, -7.0)
        ref_yh = net(xin, c)
    assert relerr(yh, ref_yh) < 1e-5, relerr(yh, ref_yh)
    assert relerr(osmp, gen_tf.squeeze(1)) < 1e-4, relerr(osmp, gen_tf.squeeze(1))
    out["gen_tf"] = gen_tf.numpy()
    out["gen_free"] = gen_free.numpy()
    out["yhat_tf.dg"] = O.digest(ref_yh, 256)
    # the small helpers SURVEY.md section 8 rows a12 / a13 name, through the reference's own functions
    from wavenet_vocoder import mixture as RM
    out["rf"] = np.array([RW.receptive_field_size(24, 4, 3), RW.receptive_field_size(6, 2, 3, lambda x: 1), RW.receptive_field_size(4, 2, 2)], dtype=np.int64)
    lens = torch.tensor([3, 5, 1])
    out["seqmask"] = RefLoss.sequence_mask(lens).numpy()
    out["seqmask6"] = RefLoss.sequence_mask(lens, 6).numpy()
    out["onehot"] = RM.to_one_hot(torch.tensor([[1, 0, 3], [2, 2, 0]]), 4).numpy()
    out["onehot_fill"] = RM.to_one_hot(torch.tensor([2, 0]), 3, 0.5).numpy()
    path = os.path.join(OUT, "wavenet_deep.npz")
    np.savez_compressed(path, **out)
    print("wavenet_deep -> %s (%.1f KB)" % (os.path.relpath(path, ROOT), os.path.getsize(path) / 1024))


def wavenet_onehot_goldens():
    """WaveNet with one-hot (mu-law) input, `scalar_input=False` (wavenet.py:116-119,177-235): teacher-forced forward and the
    gradients of a cross-entropy loss, from the reference's module.  (`forward(softmax=True)` raises a TypeError in the
    reference -- `self.softmax(x, dim=1)`, wavenet.py:233 -- so only the logits path exists to compare.)"""
    import Config  # noqa: F401
    from oracle import wavenet_oracle as W
    cfg = W.WNConfigOneHot
    from wavenet_vocoder import wavenet as RW
    net = RW.WaveNet(out_channels=cfg.out_channels, layers=cfg.layers, stacks=cfg.stacks, residual_channels=cfg.residual_channels,
                     gate_channels=cfg.gate_channels, skip_out_channels=cfg.skip_out_channels, kernel_size=cfg.kernel_size, dropout=0.0,
                     cin_channels=cfg.cin_channels, gin_channels=-1, n_speakers=None, weight_normalization=True,
                     upsample_conditional_features=True, upsample_scales=list(cfg.upsample_scales),
                     freq_axis_kernel_size=cfg.freq_axis_kernel_size, scalar_input=False)
    sd = W.wavenet_state(cfg)
    assert list(net.state_dict().keys()) == list(sd.keys())
    load_into(net, sd)
    net.train()
    B, T = 2, 64
    idx = (O.cf_uniform("wno.idx", (B, T), 0, 1) * cfg.out_channels).long().clamp(max=cfg.out_channels - 1)
    x = torch.nn.functional.one_hot(idx, cfg.out_channels).float().transpose(1, 2).contiguous()        # (B, 256, T)
    c = O.cf_uniform("wno.c", (B, cfg.cin_channels, T // 16), 0, 1)
    tgt = (O.cf_uniform("wno.tgt", (B, T), 0, 1) * cfg.out_channels).long().clamp(max=cfg.out_channels - 1)
    yh = net(x, c)
    loss = torch.nn.functional.cross_entropy(yh, tgt)
    loss.backward()
    oyh = W.wavenet_forward(sd, x, c, cfg)
    assert relerr(oyh, yh) < 1e-5, relerr(oyh, yh)
    out = OrderedDict()
    out["yhat"] = yh.detach().numpy(); out["loss"] = np.float64(loss.item())
    for k in ("first_conv.weight_v", "first_conv.weight_g", "conv_layers.2.conv.weight_v", "last_conv_layers.3.weight_v", "last_conv_layers.3.bias"):
        out["g.%s" % k] = dict(net.named_parameters())[k].grad.numpy().copy()
    path = os.path.join(OUT, "wavenet_onehot.npz")
    np.savez_compressed(path, **out)
    print("wavenet_onehot -> %s (%.1f KB)" % (os.path.relpath(path, ROOT), os.path.getsize(path) / 1024))


class WNConfigOneHotDeep:
    """oracle/wavenet_oracle.py's WNConfigDeep (the reference's depth: 24 layers / 4 stacks, dilations 1 .. 32 four times; 32 channels wide) with
    one-hot input and 256 classes.  tests/test_wavenet_onehot_synth_*.py restate it."""
    out_channels, layers, stacks, residual_channels, gate_channels, skip_out_channels = 256, 24, 4, 32, 32, 32
    kernel_size, cin_channels, upsample_scales, freq_axis_kernel_size, gin_channels, n_speakers = 3, 80, (4, 4), 3, -1, None
    scalar_input = False


def inv_cdf_draw(p, u):
    """np.random.choice(K, p=p) from ONE random_sample() draw u: cumsum in float64, normalised by its last element, searchsorted side="right"."""
    cdf = np.cumsum(np.asarray(p, dtype=np.float64))
    cdf /= cdf[-1]
    return int(min(np.searchsorted(cdf, u, side="right"), cdf.size - 1)), cdf


def wavenet_onehot_synth_goldens():
    """Sample-by-sample synthesis of the one-hot (softmax) WaveNet from the reference's own `incremental_forward` (wavenet.py:237-364) in all three
    modes it defines (:350-356).  `np.random.choice` is replaced for the duration of a run by `inv_cdf_draw` fed from closed-form uniforms, after one
    check against the unpatched function under a seeded RandomState.  Two networks, the small one and one at the reference's depth; the closed-form
    weights are sharpened (last 1x1 gain x 12, first-conv gain x 4 or more) so that what is fed back matters: both conditions are asserted here and
    again by tests/test_wavenet_onehot_synth_cpu.py from the file."""
    import Config  # noqa: F401
    from oracle import wavenet_oracle as W
    from wavenet_vocoder import wavenet as RW
    torch.set_num_threads(1)
    out = OrderedDict()
    real_choice = np.random.choice

    def make(cfg, tag, first_gain, last_gain):
        net = RW.WaveNet(out_channels=cfg.out_channels, layers=cfg.layers, stacks=cfg.stacks, residual_channels=cfg.residual_channels,
                         gate_channels=cfg.gate_channels, skip_out_channels=cfg.skip_out_channels, kernel_size=cfg.kernel_size, dropout=0.0,
                         cin_channels=cfg.cin_channels, gin_channels=-1, n_speakers=None, weight_normalization=True,
                         upsample_conditional_features=True, upsample_scales=list(cfg.upsample_scales),
                         freq_axis_kernel_size=cfg.freq_axis_kernel_size, scalar_input=False)
        sd = W.wavenet_state(cfg, tag)
        sd["first_conv.weight_g"] = sd["first_conv.weight_g"] * first_gain
        sd["last_conv_layers.3.weight_g"] = sd["last_conv_layers.3.weight_g"] * last_gain
        assert list(net.state_dict().keys()) == list(sd.keys())
        load_into(net, sd)
        return net.eval()

    def run(net, c, T, test_inputs, softmax, quantize, uniforms=None, choice=None):
        """the reference's incremental_forward; with quantize: np.random.choice <- `choice`, or the inverse-CDF draw over `uniforms` (T,), whose
        probabilities and margins are returned too"""
        seen = []

        def draw(a, p=None):
            k, cdf = inv_cdf_draw(p, float(uniforms[len(seen)]))
            seen.append((np.asarray(p, dtype=np.float32).copy(), float(np.abs(cdf - float(uniforms[len(seen)])).min())))
            return a[k]
        np.random.choice = choice if choice is not None else draw
        try:
            with torch.no_grad():
                y = net.incremental_forward(initial_input=None, c=c, g=None, T=T, test_inputs=test_inputs, tqdm=lambda z: z,
                                            softmax=softmax, quantize=quantize)
        finally:
            np.random.choice = real_choice
        return y, seen

    def rel(a, b):
        a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
        return float(np.linalg.norm(a - b) / np.linalg.norm(b))

    checked = False
    for name, cfg, tag, T, n_tags, need, stride, gains in (("small", W.WNConfigOneHot, "WN.", 64, 120, 1e-4, 1, (4,)),
                                                           ("deep", WNConfigOneHotDeep, "WNOD.", 160, 40, 3e-5, 4, (4, 8, 16, 32, 64, 128))):
        K, B = cfg.out_channels, 2
        c = O.cf_uniform("wnos.%s.c" % name, (B, cfg.cin_channels, T // 16), 0, 1)
        idx = (O.cf_uniform("wnos.%s.idx" % name, (B, T), 0, 1) * K).long().clamp(max=K - 1)
        x = torch.nn.functional.one_hot(idx, K).float().transpose(1, 2).contiguous()                   # (B, K, T)
        for fg in gains:                      # the first-conv gain is raised until what is fed back matters (the deep network is 32 wide)
            net = make(cfg, tag, fg, 12)
            p_tf = run(net, c, T, x, True, False)[0].numpy()
            p_free = run(net, c, T, x[:, :, :4].contiguous(), True, False)[0].numpy()
            dist = rel(p_free, p_tf)
            print("  %s: first-conv gain %g: max probability %.3g, free-running vs teacher-forced %.3g" % (name, fg, p_tf.max(), dist))
            if dist >= 1e-2:
                break
        assert dist >= 1e-2, dist
        l_tf = run(net, c, T, x, False, False)[0].numpy()
        assert rel(torch.softmax(torch.from_numpy(l_tf), 1).numpy(), p_tf) < 1e-6
        c1, x1 = c[:1].contiguous(), x[:1, :, :4].contiguous()
        if not checked:                       # the replacement draws what np.random.choice draws
            for seed in (3, 11):
                np.random.seed(seed)
                want = run(net, c1, T, x1, True, True, choice=real_choice)[0].argmax(1)
                np.random.seed(seed)
                got = run(net, c1, T, x1, True, True, uniforms=np.random.random_sample(T))[0].argmax(1)
                assert torch.equal(want, got), (seed, want, got)
            checked = True
        best = None
        for k in range(n_tags):               # a run whose every draw is clear of the CDF's edges: the search is needed (median margin ~ 2e-5)
            u = O.cf_uniform("wnos.%s.u%d" % (name, k), (1, T), 0, 1).numpy().reshape(T)
            y, seen = run(net, c1, T, x1, True, True, uniforms=u)
            m = min(s[1] for s in seen)
            if best is None or m > best[0]:
                best = (m, k, y.argmax(1).numpy().reshape(T), np.stack([s[0] for s in seen]), np.array([s[1] for s in seen]))
        print("  %s: best of %d uniform tags: %d, margin %.3g" % (name, n_tags, best[1], best[0]))
        assert best[0] >= need, best[0]
        steps = np.array([0, 1, T // 2, T - 1], dtype=np.int64)
        out[name + ".meta"] = np.array([B, T, K, stride, best[1]], dtype=np.int64)
        out[name + ".gains"] = np.array([fg, 12], dtype=np.float64)
        out[name + ".p_tf"] = p_tf[:, :, ::stride]
        out[name + ".logit_steps"] = steps
        out[name + ".l_tf"] = l_tf[:, :, steps]
        out[name + ".p_free"] = p_free[:, :, ::stride]
        out[name + ".feedback_dist"] = np.float64(dist)
        out[name + ".classes"] = best[2].astype(np.int64)
        out[name + ".margins"] = best[4]
        out[name + ".p_samp"] = best[3][::stride]
    path = os.path.join(OUT, "wavenet_onehot_synth.npz")
    np.savez_compressed(path, **out)
    print("wavenet_onehot_synth -> %s (%.1f KB)" % (os.path.relpath(path, ROOT), os.path.getsize(path) / 1024))
    assert os.path.getsize(path) <= 523767, "larger than the largest fixture"


class WNConfigOneHotFull:
    """oracle/wavenet_oracle.py's WNConfigFull (the reference's size: 24 layers / 4 stacks / 512 residual + gate / 256 skip channels, hop 256) with
    one-hot input and 256 classes.  tests/test_wavenet_onehot_train_gpu.py restates it."""
    out_channels, layers, stacks, residual_channels, gate_channels, skip_out_channels = 256, 24, 4, 512, 512, 256
    kernel_size, cin_channels, upsample_scales, freq_axis_kernel_size, gin_channels, n_speakers = 3, 80, (4, 4, 4, 4), 3, -1, None
    scalar_input = False


def masked_ce_fp64(yh, tgt, mask):
    """MaskedCrossEntropyLoss restated in fp64: yh (B, K, T'), tgt (B, T') classes, mask (B, T') -> sum(ce * mask) / sum(mask)"""
    ce = torch.nn.functional.cross_entropy(yh.double(), tgt.long(), reduction="none")
    return (ce * mask.double()).sum() / mask.double().sum()


def wavenet_onehot_train_goldens():
    """Training step of the one-hot (mu-law, 256-way softmax) WaveNet from the reference's own `WaveNet(scalar_input=False)` and
    `MaskedCrossEntropyLoss` (loss_functions.py:24-40) under the training convention of train.py's __train_step:
    criterion(y_hat[:, :, :-1].unsqueeze(-1), y[:, 1:], lengths=..., max_len=T - 1), where y holds the classes of the input itself (the network
    predicts its next sample).  Lengths are (T, T - 14) less the one step the convention drops, so the mask leaves rows out; the reference-width
    case has one stream, the shorter one.  Small case: outputs, loss and five gradients; reference-width case: digests only."""
    import Config  # noqa: F401
    from oracle import wavenet_oracle as W
    from wavenet_vocoder import wavenet as RW
    import warnings
    out = OrderedDict()
    for name, cfg, tag, B, T in (("small", W.WNConfigOneHot, "WN.", 2, 64), ("full", WNConfigOneHotFull, "WNOF.", 1, 1024)):
        K = cfg.out_channels
        net = RW.WaveNet(out_channels=K, layers=cfg.layers, stacks=cfg.stacks, residual_channels=cfg.residual_channels,
                         gate_channels=cfg.gate_channels, skip_out_channels=cfg.skip_out_channels, kernel_size=cfg.kernel_size, dropout=0.0,
                         cin_channels=cfg.cin_channels, gin_channels=-1, n_speakers=None, weight_normalization=True,
                         upsample_conditional_features=True, upsample_scales=list(cfg.upsample_scales),
                         freq_axis_kernel_size=cfg.freq_axis_kernel_size, scalar_input=False)
        sd = W.wavenet_state(cfg, tag)
        assert list(net.state_dict().keys()) == list(sd.keys())
        load_into(net, sd)
        net.train()
        hop = int(np.prod(cfg.upsample_scales))
        idx = (O.cf_uniform("wnot.%s.idx" % name, (B, T), 0, 1) * K).long().clamp(max=K - 1)
        x = torch.nn.functional.one_hot(idx, K).float().transpose(1, 2).contiguous()                   # (B, K, T)  data_loader_utils.py:278-281
        c = O.cf_uniform("wnot.%s.c" % name, (B, cfg.cin_channels, T // hop), 0, 1)
        y = idx.unsqueeze(-1)                                                                          # (B, T, 1)
        lengths = torch.tensor([T - 1, T - 15][2 - B:], dtype=torch.long)
        yh = net(x, c)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                                                            # reduce=False is deprecated, not gone
            loss = RefLoss.MaskedCrossEntropyLoss()(yh[:, :, :-1].unsqueeze(-1), y[:, 1:], lengths=lengths, max_len=T - 1)
        loss.backward()
        mask = RefLoss.sequence_mask(lengths, T - 1)
        assert 0 < mask.sum().item() < B * (T - 1)
        with torch.no_grad():
            oyh = W.wavenet_forward(sd, x, c, cfg)
            oloss = masked_ce_fp64(oyh[:, :, :-1], idx[:, 1:], mask)
        assert relerr(oyh, yh) < 1e-5, relerr(oyh, yh)
        assert abs(oloss.item() - loss.item()) < 1e-5 * abs(loss.item()), (oloss.item(), loss.item())
        params = dict(net.named_parameters())
        out[name + ".meta"] = np.array([B, T, K], dtype=np.int64)
        out[name + ".lengths"] = lengths.numpy()
        out[name + ".loss"] = np.float64(loss.item())
        if name == "small":
            out[name + ".idx"] = idx.numpy()
            out[name + ".yhat"] = yh.detach().numpy()
            for k in ("first_conv.weight_v", "first_conv.weight_g", "conv_layers.2.conv.weight_v", "last_conv_layers.3.weight_v", "last_conv_layers.3.bias"):
                out["%s.g.%s" % (name, k)] = params[k].grad.numpy().copy()
        else:
            out[name + ".yhat.dg"] = O.digest(yh, 256)
            for k in ("first_conv.weight_v", "first_conv.weight_g", "first_conv.bias", "conv_layers.0.conv.weight_v", "conv_layers.11.conv.weight_g",
                      "conv_layers.23.conv.weight_v", "conv_layers.12.conv1x1_skip.bias", "last_conv_layers.1.weight_v", "last_conv_layers.3.weight_v",
                      "last_conv_layers.3.bias", "upsample_conv.0.weight_v"):
                out["%s.g.%s.dg" % (name, k)] = O.digest(params[k].grad)
        print("  %s: loss %.6f, mask %d of %d rows" % (name, loss.item(), int(mask.sum().item()), B * (T - 1)))
    path = os.path.join(OUT, "wavenet_onehot_train.npz")
    np.savez_compressed(path, **out)
    print("wavenet_onehot_train -> %s (%.1f KB)" % (os.path.relpath(path, ROOT), os.path.getsize(path) / 1024))


def wavenet_g_goldens():
    """WaveNet with global (speaker) conditioning: teacher-forced forward and incremental_forward from the reference."""
    import Config  # noqa: F401
    from oracle import wavenet_oracle as W
    cfg = W.WNConfigG
    from wavenet_vocoder import wavenet as RW
    net = RW.WaveNet(out_channels=cfg.out_channels, layers=cfg.layers, stacks=cfg.stacks, residual_channels=cfg.residual_channels,
                     gate_channels=cfg.gate_channels, skip_out_channels=cfg.skip_out_channels, kernel_size=cfg.kernel_size, dropout=0.0,
                     cin_channels=cfg.cin_channels, gin_channels=cfg.gin_channels, n_speakers=cfg.n_speakers, weight_normalization=True,
                     upsample_conditional_features=True, upsample_scales=list(cfg.upsample_scales),
                     freq_axis_kernel_size=cfg.freq_axis_kernel_size, scalar_input=True)
    sd = W.wavenet_state(cfg)
    assert list(net.state_dict().keys()) == list(sd.keys()), set(net.state_dict()) ^ set(sd)
    load_into(net, sd)
    net.eval()
    out = OrderedDict()
    B, T = 2, 48
    x = O.cf_uniform("wng.x", (B, 1, T), -1, 1)
    c = O.cf_uniform("wng.c", (B, cfg.cin_channels, T // 16), 0, 1)
    g = torch.tensor([[2], [0]], dtype=torch.long)
    with torch.no_grad():
        yh = net(x, c, g)
    assert relerr(W.wavenet_forward(sd, x, c, cfg, g), yh) < 1e-5
    out["yhat"] = yh.numpy()
    Tg = 32
    cg = O.cf_uniform("wng.cg", (B, cfg.cin_channels, Tg // 16), 0, 1)
    v1 = O.cf_uniform("wng.v1", (B, Tg, 10), 1e-5, 1 - 1e-5)
    v2 = O.cf_uniform("wng.v2", (B, Tg), 1e-5, 1 - 1e-5)
    tin = O.cf_uniform("wng.tin", (B, 1, 3), -1, 1)
    seq = []
    for t in range(Tg):
        seq += [v1[:, t:t + 1, :].reshape(B, 1, 10), v2[:, t:t + 1].reshape(B, 1)]
    orig = torch.Tensor.uniform_
    torch.Tensor.uniform_ = lambda self, a=0, b=1: self.copy_(seq.pop(0).reshape(self.shape))
    try:
        with torch.no_grad():
            # B comes from test_inputs in the reference (wavenet.py:264-275): teacher-force the first 3 samples
            gen = net.incremental_forward(initial_input=None, c=cg, g=g, T=Tg, test_inputs=tin, tqdm=lambda z: z, softmax=False,
                                          quantize=False, log_scale_min=-7.0)
    finally:
        torch.Tensor.uniform_ = orig
    ogen = W.incremental_forward(sd, cg, Tg, v1, v2, cfg, test_inputs=tin, g=g)
    assert tuple(gen.shape) == (B, 1, Tg) and relerr(ogen, gen) < 1e-4, relerr(ogen, gen)
    out["gen"] = gen.numpy()
    path = os.path.join(OUT, "wavenet_g.npz")
    np.savez_compressed(path, **out)
    print("wavenet_g -> %s (%.1f KB)" % (os.path.relpath(path, ROOT), os.path.getsize(path) / 1024))


AV_CASE = dict(B=2, F=256, T=32, NF=8, num_D=2, lambda_contrast=0.1, margin=1.0)


def av_step_goldens():
    """The vision-infused step (BASELINE.json configs[2] / [3]) composed from the REFERENCE's modules -- MelEncoder,
    ImageEmbedding2, MelDecoderImage, num_D MelDiscriminators, GANLoss, L2ContrastiveLoss -- with the adaptations declared in
    oracle/viai_oracle.py (f_v tiled over the bottleneck height, avg-pool pyramid, mean of the per-scale GAN losses), at
    B2 x 256 x 32 with 8 frames per clip (bottleneck 2 x 2: the tiling is exercised)."""
    from networks import Image_Embedding as RefIE
    c = AV_CASE
    B, F_bins, T, NF, num_D = c["B"], c["F"], c["T"], c["NF"], c["num_D"]
    lam_c, margin = c["lambda_contrast"], c["margin"]
    s = O.cf_uniform("avstep.s", (B, 1, F_bins, T))
    mask = O.make_mask(B, T, "avstep.mask")
    video = O.cf_uniform("avstep.video", (B, NF, 3, 224, 224), -1, 1)
    flow = O.cf_uniform("avstep.flow", (B, NF, 2, 224, 224), -1, 1)
    RefEnc.hparams.cin_channels = F_bins
    E = load_into(RefEnc.MelEncoder(), O.encoder_state()); E.hparams.cin_channels = F_bins
    G = load_into(RefDec.MelDecoderImage(), O.decoder_variant_state("image"))
    V = load_into(RefIE.ImageEmbedding2(), O.image_embedding2_state())
    msd = O.msd_state(num_D)
    Ds = [load_into(RefDis.MelDiscriminator(), O._PrefixView(msd, "scale%d." % i)) for i in range(num_D)]
    for m in [E, G, V] + Ds:
        m.train()
    gan = RefLoss.GANLoss(use_lsgan=False, device=torch.device("cpu"))
    _cuda = torch.cuda.is_available
    torch.cuda.is_available = lambda: False          # loss_functions.py:139 calls .cuda() if available
    l2c = RefLoss.L2ContrastiveLoss(margin=margin, max_violation=False)

    def dis(x):
        outs = []
        for i, D in enumerate(Ds):
            outs.append(D(x))
            if i + 1 < num_D:
                x = torch.nn.functional.avg_pool2d(x, 3, 2, 1, count_include_pad=False)
        return outs

    def gan_ms(preds, real):
        return sum(gan(p, real) for p in preds) / float(len(preds))
    feats = E((s * mask).view(B, F_bins, T))
    f_v, _fea = V(video, flow)
    h, w = feats[-1].shape[2], feats[-1].shape[3]
    assert (h, w) == (2, 2) and tuple(f_v.shape) == (B, 256, 1, w)
    fake = G(feats, s.size(), f_v.expand(B, 256, h, w).contiguous())
    f_a = feats[-1].mean(dim=2).permute(0, 2, 1).reshape(B * w, 256)
    f_vv = f_v.reshape(B, 256, w).permute(0, 2, 1).reshape(B * w, 256)
    lc = l2c(f_a, f_vv)
    pred_real = dis(s)
    pred_fake_d = dis(fake.detach())
    loss_d = 0.5 * (gan_ms(pred_fake_d, False) + gan_ms(pred_real, True))
    loss_d.backward()
    grads_D = {"scale%d.%s" % (i, k): p.grad.clone() for i, D in enumerate(Ds) for k, p in D.named_parameters()}
    for D in Ds:
        for p in D.parameters():
            p.requires_grad_(False)
    pred_fake_g = dis(fake)
    loss_g_gan = gan_ms(pred_fake_g, True)
    loss_l1 = torch.nn.functional.l1_loss(fake, s)
    loss_g = loss_g_gan + LAMBDA_L1 * loss_l1 + lam_c * lc
    loss_g.backward()
    torch.cuda.is_available = _cuda
    # ---- the oracle's composition reproduces it
    oE, oG, oD, oV = O.encoder_state(), O.decoder_variant_state("image"), O.msd_state(num_D), O.image_embedding2_state()
    ocap = O.av_step_no_update(oE, oG, oD, oV, s, mask, video, flow, num_D, lam_c, margin)
    assert relerr(ocap["fake"], fake) < 5e-5, relerr(ocap["fake"], fake)
    assert relerr(ocap["f_v"], f_v) < 5e-5
    for k, ref in (("loss_d", loss_d), ("loss_g", loss_g), ("loss_l1", loss_l1), ("loss_contrast", lc)):
        assert abs(ocap[k].item() - ref.item()) < 5e-5 * abs(ref.item()), (k, ocap[k].item(), ref.item())
    for a, b in zip(ocap["pred_fake_g"], pred_fake_g):
        assert relerr(a, b) < 5e-5
    out = OrderedDict()
    out["meta"] = np.array([B, F_bins, T, NF, num_D], dtype=np.int64)
    out["lambda_contrast"], out["margin"] = np.float64(lam_c), np.float64(margin)
    out["fake"] = fake.detach().numpy(); out["f_v"] = f_v.detach().numpy()
    for i in range(num_D):
        out["pred_real%d" % i] = pred_real[i].detach().numpy()
        out["pred_fake_d%d" % i] = pred_fake_d[i].detach().numpy()
        out["pred_fake_g%d" % i] = pred_fake_g[i].detach().numpy()
    for k, v in (("loss_d", loss_d), ("loss_g", loss_g), ("loss_g_gan", loss_g_gan), ("loss_l1", loss_l1), ("loss_contrast", lc)):
        out[k] = np.float64(v.item())
    worst = 0.0
    for grp, named, ogr in (("grads_D", grads_D.items(), ocap["grads_D"]),
                            ("grads_E", ((k, p.grad) for k, p in E.named_parameters()), ocap["grads_E"]),
                            ("grads_G", ((k, p.grad) for k, p in G.named_parameters()), ocap["grads_G"]),
                            ("grads_V", ((k, p.grad) for k, p in V.named_parameters()), ocap["grads_V"])):
        for k, g in named:
            if g is None:
                assert ogr[k] is None, (grp, k)
                continue
            if float(g.abs().max()) < 1e-6:          # bias in front of a train-mode BatchNorm: true gradient 0
                continue
            e = relerr(ogr[k], g); worst = max(worst, e)
            assert e < 3e-2, (grp, k, e)
            out["%s.%s.dg" % (grp, k)] = O.digest(g)
    for nm, mod in (("E", E), ("G", G), ("V", V)):
        for k, v in mod.state_dict().items():
            if "running_" in k:
                out["state.%s.%s" % (nm, k)] = v.numpy().copy()
    for i, D in enumerate(Ds):
        for k, v in D.state_dict().items():
            if "running_" in k:
                out["state.D.scale%d.%s" % (i, k)] = v.numpy().copy()
    path = os.path.join(OUT, "step_av.npz")
    np.savez_compressed(path, **out)
    print("av step -> %s (%.1f KB); worst oracle-vs-reference gradient rel err %.2e" % (os.path.relpath(path, ROOT), os.path.getsize(path) / 1024, worst))


def checkpoint_structure_golden():
    """The `.pth.tar` dictionary the REFERENCE's own `utils/util.save_inpainting_checkpoint` (utils/util.py:146-162) writes for a
    model holding reference MelEncoder / MelDecoder / MelDiscriminator modules and two torch.optim.Adam optimizers after one
    step: captured as a STRUCTURE (key order, tensor shapes / dtypes, optimizer state_dict layout, python types of the scalars) in
    tests/golden/checkpoint_structure.json.  The file itself (69 MB of closed-form weights) is not kept."""
    import json
    import tempfile
    from utils import util as RefUtil
    E, G, D, optG, optD, gan = fresh(80)
    s = O.cf_uniform("s.tiny", (2, 1, 80, 32))
    ref_step(E, G, D, optG, optD, gan, s, O.make_mask(2, 32, "mask.tiny"), update=True)
    model = types.SimpleNamespace(Mel_Encoder=E, Mel_Decoder=G, netD=D, optimizer_G=optG, optimizer_D=optD)
    hp = types.SimpleNamespace(name="viai_golden", save_optimizer_state=True)

    def describe(v):
        if torch.is_tensor(v):
            return {"tensor": list(v.shape), "dtype": str(v.dtype).replace("torch.", "")}
        if isinstance(v, dict):
            return {"dict": [[k if isinstance(k, str) else int(k), describe(x)] for k, x in v.items()], "ordered": isinstance(v, OrderedDict)}
        if isinstance(v, (list, tuple)):
            return {type(v).__name__: [describe(x) for x in v]}
        return {type(v).__name__: v}
    with tempfile.TemporaryDirectory() as td:
        RefUtil.save_inpainting_checkpoint(model, 7, 3, td, 2, hparams=hp)
        files = os.listdir(td)
        assert files == ["viai_golden_checkpoint_step000000007.pth.tar"], files
        ck = torch.load(os.path.join(td, files[0]), map_location="cpu", weights_only=False)
    out = {"file_name": files[0], "checkpoint": describe(ck)}
    path = os.path.join(OUT, "checkpoint_structure.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=None, separators=(",", ":"))
    print("checkpoint structure -> %s (%.1f KB)" % (os.path.relpath(path, ROOT), os.path.getsize(path) / 1024))


def instnorm_goldens():
    """the `norm_layer=nn.InstanceNorm2d` branch of the reference constructors (Discriminator_Networks.py:10-14,
    New_Inpainting_Networks.py:12-16, Inpainting_Networks.py:50-52): reference modules, closed-form weights."""
    out = OrderedDict()
    IN = torch.nn.InstanceNorm2d
    D = RefDis.MelDiscriminator(norm_layer=IN)
    base = O.disc_state()                                     # use_bias = (norm_layer == InstanceNorm2d): the convs carry a bias (:14)
    sd = OrderedDict((k, base[k] if k in base else O.cf_uniform("in.D." + k, tuple(v.shape), -0.1, 0.1)) for k, v in D.state_dict().items())
    assert list(sd.keys()) == ["conv1.weight", "conv1.bias", "conv2_1.weight", "conv2_1.bias", "conv2_2.weight", "conv2_2.bias",
                               "conv3.weight", "conv3.bias", "conv4.weight", "conv4.bias"]
    load_into(D, sd); D.train()
    x = O.cf_uniform("in.x", (2, 1, 32, 64))
    y = D(x)
    y.mean().backward()
    out["D.out"] = y.detach().numpy()
    for k in ("conv1.weight", "conv2_2.weight", "conv3.weight", "conv4.weight", "conv4.bias", "conv3.bias"):
        out["D.g.%s.dg" % k] = O.digest(dict(D.named_parameters())[k].grad)
    blk = RefDec.TransConvBlock(32, 16, "9", nums=2, norm_layer=IN)
    bsd = OrderedDict((k, O.cf_std("in.blk." + k, tuple(v.shape), 0.1)) for k, v in blk.state_dict().items())
    assert list(bsd.keys()) == ["conv9_0.weight", "conv9_0.bias", "conv9_1.weight", "conv9_1.bias"]
    load_into(blk, bsd); blk.train()
    xb = O.cf_uniform("in.xb", (2, 32, 8, 16), -1, 1).requires_grad_(True)
    yb = blk(xb)
    yb.pow(2).mean().backward()
    out["blk.out"] = yb.detach().numpy(); out["blk.dx"] = xb.grad.numpy().copy()
    out["blk.g.conv9_1.weight"] = blk.conv9_1.weight.grad.numpy().copy()
    RefEnc.hparams.cin_channels = 96
    E = RefEnc.MelEncoder(norm_layer=IN)                      # affine=True: gamma / beta are parameters (Inpainting_Networks.py:56)
    ebase = O.encoder_state()
    esd = OrderedDict((k, ebase[k] if k in ebase else O.cf_uniform("in.E." + k, tuple(v.shape), -0.1, 0.1)) for k, v in E.state_dict().items())
    assert "conv1.bias" in esd and "bn1.weight" in esd and "bn1.running_mean" not in esd
    load_into(E, esd); E.train()
    xe = O.cf_uniform("in.xe", (2, 96, 32))
    fe = E(xe)
    sum(f.pow(2).mean() for f in fe).backward()
    for i in (0, 3):
        out["E.feat%d" % i] = fe[i].detach().numpy()
    out["E.g.bn2.weight"] = E.bn2.weight.grad.numpy().copy(); out["E.g.conv3.weight.dg"] = O.digest(E.conv3.weight.grad)
    path = os.path.join(OUT, "instnorm.npz")
    np.savez_compressed(path, **out)
    print("instnorm -> %s (%.1f KB)" % (os.path.relpath(path, ROOT), os.path.getsize(path) / 1024))


def loader_goldens():
    """The callers in front of / behind the path that round 1 left unpinned, now driven through the
    REFERENCE's own functions:

      * `Data_loaders.audio_loader.sample_data_new` (:156-245: frame normalisation (px - 127) / 128, horizontal flip, random crop,
        (N, C, H, W) transpose) and `collate_fn` (:432-532: mel / audio window slicing `3 + 4 start`, zero padding, (B, C, T)
        transposes);
      * `utils.audio._denormalize` / `_db_to_amp` / `_amp_to_db` / `_normalize` / `lws_num_frames` / `lws_pad_lr` (:90-144).

    Both modules import packages that are absent here (nnmnkwii, keras, cv2, lws, librosa).  None of the functions above calls into
    nnmnkwii / keras / lws / librosa, so empty stand-in modules make the import succeed; `cv2` is a HARNESS that feeds synthetic
    closed-form frames: `imread` returns the frame of that file name, `cvtColor` reverses the channel axis (BGR -> RGB), `resize`
    asserts the frame already has the requested size (so no interpolation is involved).  numpy's RNG is recorded, so the crop / flip /
    start draws of the reference are part of the fixture."""
    import tempfile
    from oracle import pipeline_oracle as P
    for name in ("nnmnkwii", "nnmnkwii.datasets", "keras", "keras.utils", "keras.utils.np_utils", "lws", "librosa", "librosa.filters"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["nnmnkwii.datasets"].FileSourceDataset = object
    sys.modules["nnmnkwii.datasets"].FileDataSource = object
    sys.modules["keras.utils"].np_utils = sys.modules["keras.utils.np_utils"]
    cv2 = sys.modules["cv2"]
    R = 256

    def frame(path, gray):
        idx = int(os.path.basename(path).split(".")[0])
        kind = os.path.basename(os.path.dirname(path))
        t = O.cf_uniform("ld.%s.%d" % (kind, idx), (R, R) if gray else (R, R, 3), 0, 256).numpy()
        return np.clip(np.floor(t), 0, 255).astype(np.uint8)
    cv2.imread = lambda path, flag=1: frame(path, flag == 0)
    cv2.COLOR_BGR2RGB = 4
    cv2.cvtColor = lambda img, code: img[..., ::-1]

    def resize(img, size):
        assert tuple(img.shape[:2]) == (size[1], size[0]), "harness frames are generated at the requested size"
        return img
    cv2.resize = resize
    from Data_loaders import audio_loader as RL
    from utils import audio as RA
    hp = RL.hparams
    out = OrderedDict()
    with tempfile.TemporaryDirectory() as td:
        n_frames = 180
        for sub in ("flow_x_crop", "flow_y_crop", "image_crop"):
            os.makedirs(os.path.join(td, sub))
            for i in range(n_frames):
                open(os.path.join(td, sub, "%d.jpg" % (i + 1)), "w").close()
        draws = []
        orig = np.random.randint

        def rec(*a, **k):
            v = orig(*a, **k)
            draws.append(int(v))
            return v
        np.random.seed(7)
        np.random.randint = rec
        try:
            video, flow, start = RL.sample_data_new(td, train=True, hparams=hp)
        finally:
            np.random.randint = orig
    use = video.shape[1]
    assert video.shape == (hp.load_num, use, 3, 224, 224) and flow.shape == (hp.load_num, use, 2, 224, 224) and use == 52
    crop_x, crop_y, flip = draws[-3], draws[-2], draws[-1]
    out["starts"] = np.array(start, dtype=np.int64)
    out["crop_flip"] = np.array([crop_x, crop_y, flip], dtype=np.int64)
    out["video.dg"] = O.digest(torch.from_numpy(video), 256); out["flow.dg"] = O.digest(torch.from_numpy(flow), 256)
    out["video_first"] = video[0, 0].astype(np.float32); out["flow_last"] = flow[-1, -1].astype(np.float32)
    # the oracle's frames_prep on the same frames (read the harness way: RGB = reversed BGR; flow = (x, y) planes)
    for ln in (0, hp.load_num - 1):
        for i in (0, use - 1):
            item = start[ln] + i + 1
            rgb = frame(os.path.join("image_crop", "%d.jpg" % item), False)[..., ::-1]
            fl = np.stack((frame(os.path.join("flow_x_crop", "%d.jpg" % item), True), frame(os.path.join("flow_y_crop", "%d.jpg" % item), True)), -1)
            assert np.abs(P.frames_prep(rgb, 224, crop_x, crop_y, flip) - video[ln, i]).max() < 1e-6
            assert np.abs(P.frames_prep(fl, 224, crop_x, crop_y, flip) - flow[ln, i]).max() < 1e-6
    # ---- collate_fn: two utterances, load_num windows each
    batch, mels, wavs = [], [], []
    for u in range(2):
        T_mel = 3 + 4 * (max(start) + use) + 5 + 11 * u
        c = O.cf_uniform("ld.c%d" % u, (T_mel, 80), 0, 1).numpy()
        x = O.cf_uniform("ld.x%d" % u, (T_mel * hp.hop_size,), -1, 1).numpy()
        mels.append(c); wavs.append(x)
        batch.append((x, c, video, flow, start, None, "utt%d" % u))
    vb, fb, cb, xb, yb, gb, lens, paths = RL.collate_fn(batch)
    assert tuple(cb.shape) == (4, 80, 208) and tuple(xb.shape) == (4, 1, 208 * hp.hop_size) and gb is None
    k = 0
    for u in range(2):
        oc, ox = P.slice_clips(mels[u], wavs[u], start, use, hp.hop_size)
        assert np.array_equal(oc, cb[k:k + 2].numpy()) and np.array_equal(ox, xb[k:k + 2].numpy())
        k += 2
    assert torch.equal(yb.squeeze(-1), xb.squeeze(1)) and lens.tolist() == [208 * hp.hop_size] * 4
    out["collate.c.dg"] = O.digest(cb, 256); out["collate.x.dg"] = O.digest(xb, 256)
    out["collate.c_clip1"] = cb[1].numpy()
    # ---- utils/audio.py plain-numpy helpers
    S = O.cf_uniform("ld.S", (80, 64), -0.2, 1.2).numpy()
    out["inv_mel"] = RA._db_to_amp(RA._denormalize(S.astype(np.float64)))              # fp64 input: the function's exact arithmetic
    out["inv_mel_f32"] = RA._db_to_amp(RA._denormalize(S)).astype(np.float64)           # fp32 input, as a network output would arrive
    assert np.allclose(P.inv_mel_amplitude(S, RA.hparams.min_level_db), out["inv_mel"], rtol=1e-12)
    assert np.allclose(out["inv_mel_f32"], out["inv_mel"], rtol=2e-5)
    amp = (10.0 ** O.cf_uniform("ld.amp", (80, 64), -7, 1).double().numpy())
    out["amp_to_db_norm"] = RA._normalize(RA._amp_to_db(amp) - RA.hparams.ref_level_db)
    from oracle import audio_oracle as AO
    assert np.allclose(AO.normalize(AO.amp_to_db(amp, RA.hparams.min_level_db) - RA.hparams.ref_level_db, RA.hparams.min_level_db), out["amp_to_db_norm"], rtol=1e-12, atol=1e-15)
    tab = []
    for length in (1, 255, 256, 257, 1024, 65536, 66560, 66561, 100000):
        x = np.zeros(length)
        tab.append([length, RA.lws_num_frames(length, 1024, 256)] + list(RA.lws_pad_lr(x, 1024, 256)) + [RA.lws_num_frames(length, 1024, 320)] + list(RA.lws_pad_lr(x, 1024, 320)))
        assert tab[-1][1] == AO.lws_num_frames(length, 1024, 256) and tuple(tab[-1][2:4]) == tuple(AO.lws_pad_lr(length, 1024, 256))
    out["lws_table"] = np.array(tab, dtype=np.int64)
    out["min_level_db"], out["ref_level_db"] = np.float64(RA.hparams.min_level_db), np.float64(RA.hparams.ref_level_db)
    path = os.path.join(OUT, "loader.npz")
    np.savez_compressed(path, **out)
    print("loader -> %s (%.1f KB); starts %s crop/flip %s" % (os.path.relpath(path, ROOT), os.path.getsize(path) / 1024, start, (crop_x, crop_y, flip)))


def adam_goldens():
    """torch.optim.Adam known-answer vectors (what the missing AudioModel's
    optimizer_G/optimizer_D are, utils/util.py:149-150)."""
    out = OrderedDict()
    c = O.StepConfig
    p = torch.nn.Parameter(O.cf_uniform("adam.p", (4096,), -1, 1))
    opt = torch.optim.Adam([p], lr=c.lr, betas=(c.beta1, c.beta2), eps=c.eps)
    sd = OrderedDict(p=p.detach().clone())
    oopt = O.Adam(sd, c)
    for t in range(3):
        g = O.cf_uniform("adam.g%d" % t, (4096,), -1, 1) * (10.0 ** O.cf_uniform("adam.e%d" % t, (4096,), -9, 0))
        p.grad = g.clone()
        opt.step()
        oopt.step(sd, {"p": g})
        out["p_after_%d" % (t + 1)] = p.detach().numpy().copy()
        assert relerr(sd["p"], p.detach()) < 1e-6
    path = os.path.join(OUT, "adam.npz")
    np.savez_compressed(path, **out)
    print("adam -> %s (%.1f KB)" % (os.path.relpath(path, ROOT), os.path.getsize(path) / 1024))


def layer_goldens():
    """Per-layer known-answer vectors from torch.nn layers the reference uses."""
    out = OrderedDict()
    # ConvTranspose2d stride 1 pad (0,1) (New_Inpainting_Networks.py:53)
    x = O.cf_uniform("lg.x", (2, 32, 3, 8), -1, 1)
    w = O.cf_std("lg.w", (32, 32, 3, 3), 0.1)
    b = O.cf_uniform("lg.b", (32,), -0.1, 0.1)
    m = torch.nn.ConvTranspose2d(32, 32, 3, 1, (0, 1))
    m.weight.data.copy_(w); m.bias.data.copy_(b)
    out["convT_p01"] = m(x).detach().numpy()
    m = torch.nn.Conv2d(32, 64, (3, 3), stride=(2, 1), padding=(1, 1), bias=False)
    w2 = O.cf_std("lg.w2", (64, 32, 3, 3), 0.1)
    m.weight.data.copy_(w2)
    out["conv_s21"] = m(x).detach().numpy()
    out["bilinear_3x8_to_7x20"] = torch.nn.functional.interpolate(
        x, size=[7, 20], mode="bilinear", align_corners=True).numpy()
    assert relerr(O.bilinear_ac(x, (7, 20)), torch.from_numpy(out["bilinear_3x8_to_7x20"])) < 1e-6
    # GANLoss (loss_functions.py:79-104), BCE and MSE, incl. the log clamp
    p = torch.tensor([[0.0, 1.0, 0.25, 0.999999, 1e-30, 0.5]])
    for lsgan in (False, True):
        gan = RefLoss.GANLoss(use_lsgan=lsgan, device=torch.device("cpu"))
        for real in (False, True):
            v = gan(p, real).item()
            out["gan_%s_%s" % ("mse" if lsgan else "bce", "real" if real else "fake")] = np.float64(v)
            assert abs(O.gan_loss(p, real, lsgan).item() - v) <= 1e-6 * max(1, abs(v))
    f1 = O.cf_uniform("lg.f1", (6, 256), -1, 1)
    f2 = O.cf_uniform("lg.f2", (6, 256), -1, 1)
    _cuda = torch.cuda.is_available
    torch.cuda.is_available = lambda: False          # loss_functions.py:139 calls .cuda() if available
    for mv in (False, True):
        v = RefLoss.L2ContrastiveLoss(margin=12.0, max_violation=mv)(f1, f2).item()
        out["l2c_mv%d" % mv] = np.float64(v)
        assert abs(O.l2_contrastive(f1, f2, 12.0, mv).item() - v) <= 1e-5 * abs(v)
    torch.cuda.is_available = _cuda
    path = os.path.join(OUT, "layers.npz")
    np.savez_compressed(path, **out)
    print("layers -> %s (%.1f KB)" % (os.path.relpath(path, ROOT), os.path.getsize(path) / 1024))


def pipeline_goldens():
    """The callers either side of the path: lr schedules, EMA, retrieval metrics, produced by
    the reference's own functions and checked against oracle/pipeline_oracle.py."""
    from utils import lrschedule as RefLR
    from utils import util as RefUtil
    from oracle import pipeline_oracle as P
    out = {}
    steps = np.array([0, 1, 7, 1999, 2000, 2001, 49999, 50000, 123456, 1000000], dtype=np.int64)
    out["lr_steps"] = steps
    out["lr_noam"] = np.array([RefLR.noam_learning_rate_decay(1e-3, int(s), 2000) for s in steps])
    out["lr_step"] = np.array([RefLR.step_learning_rate_decay(1e-3, int(s), 0.98, 50000) for s in steps])
    out["lr_cyclic"] = np.array([RefLR.cyclic_cosine_annealing(1e-3, int(s), 200000, 5) for s in steps])
    for k, f in (("lr_noam", lambda s: P.noam_learning_rate_decay(1e-3, s, 2000)),
                 ("lr_step", lambda s: P.step_learning_rate_decay(1e-3, s, 0.98, 50000)),
                 ("lr_cyclic", lambda s: P.cyclic_cosine_annealing(1e-3, s, 200000, 5))):
        assert np.allclose(out[k], [f(int(s)) for s in steps], rtol=1e-14, atol=0)
    # ExponentialMovingAverage (loss_functions.py:65-76): 5 updates at decay 0.9999 and 0.9
    for decay in (0.9999, 0.9):
        ema = RefLoss.ExponentialMovingAverage(decay)
        ema.register("w", O.cf_uniform("ema.w0", (3, 50), -1, 1))
        sh = O.cf_uniform("ema.w0", (3, 50), -1, 1).numpy()
        for i in range(5):
            x = O.cf_uniform("ema.x%d" % i, (3, 50), -1, 1)
            ema.update("w", x)
            sh = P.ema_update(sh, x.numpy(), decay)
        out["ema_%g" % decay] = ema.shadow["w"].numpy()
        assert np.abs(sh - out["ema_%g" % decay]).max() <= 1e-7
    # L2retrieval (utils/util.py:99-121): captions = noisy copies of the clips, so ranks are spread out
    W = O.cf_uniform("ret.W", (4, 256), -1, 1).numpy()                 # embeddings on a 4-d subspace: ranks spread out
    z = O.cf_uniform("ret.z", (96, 4), -1, 1).numpy()
    clips = (z @ W).astype(np.float32)
    caps = ((z + 0.5 * O.cf_uniform("ret.e", (96, 4), -1, 1).numpy()) @ W).astype(np.float32)
    metrics, (ranks, top1) = RefUtil.L2retrieval(clips, caps, return_ranks=True)
    out["ret_metrics"] = np.array(metrics, dtype=np.float64)
    out["ret_ranks"], out["ret_top1"] = ranks.astype(np.int64), top1.astype(np.int64)
    m2, r2, t2 = P.l2_retrieval(clips, caps)
    assert np.array_equal(r2, ranks) and np.array_equal(t2, top1) and np.allclose(m2, metrics)
    assert len(set(ranks.tolist())) > 5, "degenerate retrieval golden"
    path = os.path.join(OUT, "pipeline.npz")
    np.savez_compressed(path, **out)
    print("pipeline -> %s (%.1f KB)" % (os.path.relpath(path, ROOT), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    if "--pipeline-only" in sys.argv:
        pipeline_goldens()
        sys.exit(0)
    if "--wavenet-g-only" in sys.argv:
        wavenet_g_goldens()
        sys.exit(0)
    if "--wavenet-onehot-only" in sys.argv:
        wavenet_onehot_goldens()
        sys.exit(0)
    if "--wavenet-onehot-synth-only" in sys.argv:
        wavenet_onehot_synth_goldens()
        sys.exit(0)
    if "--wavenet-onehot-train-only" in sys.argv:
        torch.set_num_threads(os.cpu_count())
        wavenet_onehot_train_goldens()
        sys.exit(0)
    if "--ganloss-soft-only" in sys.argv:
        ganloss_soft_goldens()
        sys.exit(0)
    if "--chain-only" in sys.argv:
        chain_goldens()
        sys.exit(0)
    if "--wavenet-deep-only" in sys.argv:
        wavenet_deep_goldens()
        sys.exit(0)
    if "--wavenet-full-only" in sys.argv:
        torch.set_num_threads(os.cpu_count())
        wavenet_full_goldens()
        sys.exit(0)
    if "--loader-only" in sys.argv:
        loader_goldens()
        sys.exit(0)
    if "--instnorm-only" in sys.argv:
        instnorm_goldens()
        sys.exit(0)
    if "--checkpoint-only" in sys.argv:
        checkpoint_structure_golden()
        sys.exit(0)
    if "--av-step-only" in sys.argv:
        torch.set_num_threads(os.cpu_count())
        av_step_goldens()
        sys.exit(0)
    if "--cfg2-only" in sys.argv:
        torch.set_num_threads(os.cpu_count())
        run_case("cfg2", 16, 256, 256, 1, full=False)  # BASELINE.json configs[1], the benchmark size (digests only)
        sys.exit(0)
    torch.set_num_threads(os.cpu_count())
    layer_goldens()
    pipeline_goldens()
    adam_goldens()
    av_goldens()
    resnet_goldens()
    wavenet_goldens()
    wavenet_g_goldens()
    wavenet_full_goldens()
    wavenet_onehot_goldens()
    wavenet_onehot_synth_goldens()
    wavenet_onehot_train_goldens()
    wavenet_deep_goldens()
    av_step_goldens()
    instnorm_goldens()
    loader_goldens()
    checkpoint_structure_golden()
    run_case("tiny", 2, 80, 32, 3, full=True)        # smallest valid shape
    chain_goldens()
    ganloss_soft_goldens()
    run_case("cfg1", 4, 128, 128, 1, full=False)      # BASELINE.json configs[0]
    if "--cfg2" in sys.argv:
        run_case("cfg2", 16, 256, 256, 1, full=False)  # configs[1]; ~1 min on 8 cores
