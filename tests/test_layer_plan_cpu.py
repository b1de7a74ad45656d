"""The host-side decisions of viai_amd/networks.py, pinned without a GPU.  Nothing is launched; only shapes go in.

  * `networks.plan_layer` -- route, the act / training / out_p16 handed to ops.conv_bn_act, and the passes that run behind the call -- is compared
    with the decisions `fused_layer` spelled out inline before it (written out below as they stood, as the specification) on every fused_layer
    call of E, G (MelDecoder and MelDecoderImage), D and one ResNet-18, built by hand as their forward_nhwc builds them, at the step's shape
    (B 16, F = T = 256, T / 4 frames of 224 x 224 per clip) and a small one (B 2, F = T = 32: the encoder's last map has one row there, so its
    AvgPool((3, 1)) leaves none -- only arithmetic on shapes happens here), crossed with the five switches, bn.training, BatchNorm and
    InstanceNorm holders (every call once more with an nn.InstanceNorm2d of its width in place of its norm), and `next_conv` given and None.
  * `takes_p16`, `wgrad_takes_p16`, `out_shape` answer as ops.conv_takes_p16, ops.conv_wgrad_takes_p16 and viai_conv2d_out_hw do.
  * a residual with an activation other than ReLU / none is refused; fused_layer does not call itself; one ops.conv_bn_act call for 2-D holders.
"""
import ast
import inspect
import itertools
import types

import pytest
import torch.nn as nn

from test_conv_routes_cpu import lib  # noqa: F401  (the fixture: the built library)

ACT_NONE, ACT_RELU, ACT_LRELU = 0, 1, 2
BOOLS = (False, True)
SWITCHES = ("FUSE_BN_TAIL", "P16_TWIN", "P16", "F16_BACKWARD", "FUSE_BN_UP")
SHAPES = ((16, 256, 256), (2, 32, 32))


def spec_fused_layer(N_, ops, x_shape, conv, bn, act, *, training=True, has_xmask=False, has_residual=False, pool=None, upsample=None, next_conv=None):
    """fused_layer before plan_layer: (route, act and training and out_p16 of its ops.conv_bn_act call, the passes behind that call)"""
    transposed = isinstance(conv, nn.ConvTranspose2d)
    x = types.SimpleNamespace(shape=tuple(x_shape))
    if upsample is not None:
        up = (int(upsample[0]), int(upsample[1]))
        if not has_residual and pool is None and not has_xmask and ops.upsample_fusable(x, conv.weight, conv.bias, bn, transposed, act, up):
            p16 = (next_conv is not None and isinstance(bn, nn.modules.batchnorm._BatchNorm) and bn.training
                   and N_.takes_p16((x.shape[0], up[0], up[1], conv.out_channels), next_conv))
            return "up", act, bn.training, p16, ()
        # ops.bilinear_ac(fused_layer(... without upsample and WITHOUT next_conv ...), up)
        inner = spec_fused_layer(N_, ops, x_shape, conv, bn, act, training=training, has_xmask=has_xmask, has_residual=has_residual, pool=pool)
        return inner[:4] + (inner[4] + ("bilinear_ac",),)
    behind = ((("add_relu" if act == ACT_RELU else "add",) if has_residual else ()) + (("maxpool",) if pool is not None else ()))
    if isinstance(bn, nn.InstanceNorm2d):
        return "instance", (ACT_NONE if has_residual else act), True, False, behind
    if N_.FUSE_BN_TAIL and isinstance(bn, nn.modules.batchnorm._BatchNorm) and act in (ACT_RELU, ACT_NONE) and (has_residual or pool is not None):
        oshape = N_.out_shape(x.shape, conv)
        if pool is not None:
            oshape = (oshape[0], (oshape[1] + 2 * pool[2] - pool[0]) // pool[1] + 1, (oshape[2] + 2 * pool[2] - pool[0]) // pool[1] + 1, oshape[3])
        twin = N_.P16_TWIN and next_conv is not None and bn.training and (N_.takes_p16(oshape, next_conv) or N_.wgrad_takes_p16(oshape, next_conv))
        return "tail", act, bn.training, twin, ()
    p16 = (next_conv is not None and not has_residual and pool is None and isinstance(bn, nn.modules.batchnorm._BatchNorm) and bn.training
           and N_.takes_p16(N_.out_shape(x.shape, conv), next_conv))
    return "plain", (ACT_NONE if has_residual else act), (bn.training if bn is not None else training), p16, behind


def _calls(N_, B, F, T):
    """every fused_layer call of the networks, as (x_shape, conv, bn, act, keywords but next_conv, follower).  `follower` is the `next_conv`
    the network passes; where it passes none (E, the video head of G, the downsample convs, a block in front of the skip concat) the conv
    that follows anyway, so that every call is planned with a `next_conv` given and with None (None only: E.conv5, the last join)."""
    out = []

    def add(x_shape, conv, bn, act, follower=None, **kw):
        out.append((tuple(x_shape), conv, bn, act, kw, follower))
        return N_.out_shape(x_shape, conv)

    # E (MelEncoder.forward_nhwc): no next_conv -- each map is also a skip source of the decoder
    E = N_.MelEncoder()
    s, net = (B, F, T, 1), []
    for i in range(5):
        follower = E._modules["conv%d" % (i + 2)] if i < 4 else None
        s = add(s, E._modules["conv%d" % (i + 1)], E._modules["bn%d" % (i + 1)], ACT_LRELU, follower, has_xmask=(i == 0))
        net.append(s)
    net[-1] = (s[0], s[1] // 3, s[2], s[3])              # ops.avgpool_h(net[-1], 3)
    sizes = [net[-1 - i][1:3] for i in range(1, 5)] + [(F, T)]

    def blocks(G, s):
        for i in range(1, 5):                            # MelDecoder.forward_nhwc
            blk = G._modules["convblock%d" % (i + 1)]
            nb = G._modules["convblock%d" % (i + 2)] if i + 1 < 5 else None
            nxt = nb._modules["conv%s_0" % nb.name] if nb is not None else G.conv6_1       # (the network passes None when i + 1 == skip_at)
            for j in range(blk.nums):                    # TransConvBlock.forward_nhwc (x2 = the skip map on j == 0 when i == skip_at: the plan does not read it)
                conv, bn = blk._modules["conv%s_%d" % (blk.name, j)], blk._modules["conv%s_%d_bn" % (blk.name, j)]
                last = j == blk.nums - 1
                n_ = nxt if last else blk._modules["conv%s_%d" % (blk.name, j + 1)]
                s = add(s, conv, bn, ACT_RELU, n_, upsample=sizes[i] if last else None)
                if last:
                    s = (s[0], sizes[i][0], sizes[i][1], s[3])

    G = N_.MelDecoder()                                  # MelDecoder._head
    nb0 = G.convblock2._modules["conv2_0"]
    s = add(net[-1], G.deconv1_1, G.deconv1_1_bn, ACT_RELU, G.deconv1_2)
    s = add(s, G.deconv1_2, G.deconv1_2_bn, ACT_RELU, nb0, upsample=sizes[0])
    blocks(G, (s[0], sizes[0][0], sizes[0][1], s[3]))
    GI = N_.MelDecoderImage()                            # MelDecoderImage._head_av (x2 = the video feature), then ops.bilinear_ac and the same blocks
    s = add(net[-1], GI.deconv1_1_1, GI.deconv1_1_1_bn, ACT_RELU, GI.deconv1_2)
    s = add(s, GI.deconv1_2, GI.deconv1_2_bn, ACT_RELU, GI.convblock2._modules["conv2_0"])
    blocks(GI, (s[0], sizes[0][0], sizes[0][1], s[3]))

    D = N_.MelDiscriminator()                            # MelDiscriminator.forward_nhwc (conv3 -> conv4 is the pair)
    s = add((B, F, T, 1), D.conv1, D.bn1, ACT_LRELU, D.conv2_1)
    s = add(s, D.conv2_1, D.norm_1, ACT_LRELU, D.conv2_2)
    add(s, D.conv2_2, D.norm_2, ACT_LRELU, D.conv3)

    R = N_.ImageResnet18()                               # ResNet.forward / BasicBlock.forward_nhwc
    blks = [blk for layer in (R.layer1, R.layer2, R.layer3, R.layer4) for blk in layer]
    assert len(blks) == 8
    s = add((B * (T // 4), 224, 224, 4), R.conv1, R.bn1, ACT_RELU, blks[0].conv1, pool=(3, 2, 1))
    s = N_.pooled_shape(s, (3, 2, 1))
    for i, blk in enumerate(blks):
        nxt = blks[i + 1].conv1 if i + 1 < len(blks) else None
        h = add(s, blk.conv1, blk.bn1, ACT_RELU, blk.conv2)
        if blk.downsample is not None:
            add(s, blk.downsample[0], blk.downsample[1], ACT_NONE, nxt)
        s = add(h, blk.conv2, blk.bn2, ACT_RELU, nxt, has_residual=True)
    return out


@pytest.fixture(scope="module")
def calls():
    from viai_amd import networks as N_
    return [c for shape in SHAPES for c in _calls(N_, *shape)]


def test_calls_are_the_networks_layers(calls):
    """5 (E) + 2 + 13 (G) + 2 + 13 (G with the video feature) + 3 (D) + 1 + 8 * 2 + 3 (ResNet-18: stem, blocks, downsamples) per shape"""
    assert len(calls) == 2 * 58
    assert sum(1 for c in calls if c[4].get("pool")) == 2 and sum(1 for c in calls if c[4].get("has_residual")) == 16
    assert sum(1 for c in calls if c[4].get("upsample")) == 2 * 9 and sum(1 for c in calls if c[4].get("has_xmask")) == 2


def test_plan_agrees_with_the_decisions_it_replaced(lib, calls, monkeypatch):  # noqa: F811
    from viai_amd import networks as N_, ops
    assert (ops.ACT_NONE, ops.ACT_RELU, ops.ACT_LRELU) == (ACT_NONE, ACT_RELU, ACT_LRELU)
    inorms = {}
    routes, p16_seen, resize_seen, rows = set(), set(), set(), 0
    for switches in itertools.product(BOOLS, repeat=len(SWITCHES)):
        for name, v in zip(SWITCHES, switches):
            monkeypatch.setattr(N_ if hasattr(N_, name) else ops, name, v)
        for (x_shape, conv, bn, act, kw, follower), train, instance, given in itertools.product(calls, BOOLS, BOOLS, BOOLS):
            norm = inorms.setdefault(conv, nn.InstanceNorm2d(conv.out_channels)) if instance else bn
            norm.train(train)
            kw = dict(kw, next_conv=(follower if given else None))
            want = spec_fused_layer(N_, ops, x_shape, conv, norm, act, **kw)
            plan = N_.plan_layer(x_shape, conv, norm, act, **kw)
            assert (plan.route, plan.act, plan.training, plan.out_p16, plan.behind) == want, (switches, x_shape, conv, norm, kw)
            assert plan.geom == N_._conv_geom(conv) and plan.geom.ok
            routes.add(plan.route)
            p16_seen.add((plan.route, plan.out_p16))
            if kw.get("upsample") is not None:
                resize_seen.add("inside" if plan.route == "up" else "behind")
                assert ("bilinear_ac" in plan.behind) == (plan.route != "up")
            rows += 1
    assert rows == 2 ** 5 * len(calls) * 8
    assert routes == {"instance", "tail", "up", "plain"}
    assert p16_seen == {("instance", False)} | {(r, p) for r in ("plain", "up", "tail") for p in BOOLS}, sorted(p16_seen)
    assert resize_seen == {"inside", "behind"}


def test_holder_questions_answer_as_the_library_does(lib, calls):  # noqa: F811
    from viai_amd import networks as N_, ops
    seen = set()
    for x_shape, conv, _, _, _, _ in calls:
        if 0 in x_shape:
            continue                                     # (the small shape's bottleneck: no rows, no descriptor)
        k, s, p = [(v, v) if isinstance(v, int) else tuple(v) for v in (conv.kernel_size, conv.stride, conv.padding)]
        tr = isinstance(conv, nn.ConvTranspose2d)
        assert N_._conv_geom(conv) == (k, s, p, tr, True)
        d = ops._layer_desc(x_shape, 0, conv.weight, k, s, p, tr)
        assert N_.out_shape(x_shape, conv) == (x_shape[0], d["OH"], d["OW"], conv.out_channels), (x_shape, conv)
        if x_shape[3] % 32 == 0:
            assert N_.takes_p16(x_shape, conv) == ops.conv_takes_p16(x_shape, conv.weight, k, s, p, tr), (x_shape, conv)
            assert N_.wgrad_takes_p16(x_shape, conv) == (not tr and ops.conv_wgrad_takes_p16(x_shape, conv.weight, k, s, p, tr)), (x_shape, conv)
            seen.add((N_.takes_p16(x_shape, conv), N_.wgrad_takes_p16(x_shape, conv)))
    assert {a for a, _ in seen} == {False, True} and {b for _, b in seen} == {False, True}
    # what the HIP path does not take: groups, dilation, a strided transposed conv -- refused before any descriptor is made
    for bad in (nn.Conv2d(64, 64, 3, 1, 1, groups=2), nn.Conv2d(64, 64, 3, 1, 2, dilation=2), nn.ConvTranspose2d(64, 64, 3, 2, 1)):
        assert not N_._conv_geom(bad).ok and N_.takes_p16((2, 16, 16, 64), bad) is False and N_.wgrad_takes_p16((2, 16, 16, 64), bad) is False
    assert N_.pooled_shape((2, 112, 112, 64), (3, 2, 1)) == (2, 56, 56, 64) and N_.pooled_shape((2, 16, 15, 64), (3, 2, 1)) == (2, 8, 8, 64)
    with pytest.raises(NotImplementedError):
        N_.plan_layer((2, 16, 16, 64), nn.ConvTranspose2d(64, 64, 3, 2, 1), nn.BatchNorm2d(64), ACT_RELU)


@pytest.mark.parametrize("norm", [nn.BatchNorm2d, nn.InstanceNorm2d, None])
@pytest.mark.parametrize("tail", BOOLS)
def test_a_residual_takes_relu_or_no_activation(norm, tail, monkeypatch):
    """the unfused routes used to run such a layer without its activation and return out + residual"""
    from viai_amd import networks as N_, ops
    monkeypatch.setattr(N_, "FUSE_BN_TAIL", tail)
    conv, bn = nn.Conv2d(32, 32, 3, 1, 1), norm(32) if norm else None
    for act in (ops.ACT_LRELU, ops.ACT_SIGMOID):
        for kw in ({}, {"upsample": (32, 32)}, {"pool": (3, 2, 1)}):
            with pytest.raises(ValueError):
                N_.plan_layer((2, 16, 16, 32), conv, bn, act, has_residual=True, **kw)
    for act in (ops.ACT_RELU, ops.ACT_NONE):
        N_.plan_layer((2, 16, 16, 32), conv, bn, act, has_residual=True)


def test_one_executor_in_the_source():
    """fused_layer plans and runs: it does not call itself, and networks.py has one ops.conv_bn_act call for 2-D holders (conv1d_layer and
    linear_layer, the 1-D holders, have one each)"""
    from viai_amd import networks as N_

    def calls_of(fn_src, owner, name):
        return [n for n in ast.walk(ast.parse(fn_src)) if isinstance(n, ast.Call)
                and (isinstance(n.func, ast.Attribute) and isinstance(n.func.value, ast.Name) and n.func.value.id == owner and n.func.attr == name
                     if owner else isinstance(n.func, ast.Name) and n.func.id == name)]
    assert not calls_of(inspect.getsource(N_.fused_layer), None, "fused_layer")
    assert len(calls_of(inspect.getsource(N_.plan_layer), None, "plan_layer")) == 0
    total = len(calls_of(inspect.getsource(N_), "ops", "conv_bn_act"))
    one_d = sum(len(calls_of(inspect.getsource(f), "ops", "conv_bn_act")) for f in (N_.conv1d_layer, N_.linear_layer))
    assert (total, one_d) == (3, 2)
    assert len(calls_of(inspect.getsource(N_.fused_layer), "ops", "conv_bn_act")) == 1
