"""What the inference tests share: the clip shapes AudioModel.test() is pinned at, and the generator's conv descriptors at a shape.

INFERENCE_SHAPES are (B, F, T) mel batches chosen for the kernels and tails their layers reach (tests/test_inference_routes_cpu.py holds the
list to that; tests/test_inference_launches_gpu.py runs it).  At none of them does every tile divide evenly, which is what the timed step's
16 x 256 x 256 never shows.

generator_layers(B, F, T) walks a MelEncoder and a MelDecoder holder on the CPU in the order of their forward (networks.MelEncoder.forward_nhwc,
MelDecoder.forward_nhwc: head, four blocks each resized to the encoder map of its scale, the Cout = 1 pair) and derives every conv's 17-field
descriptor with networks.out_shape.  Nothing is launched and no descriptor is written down by hand.
"""
import collections

INFERENCE_SHAPES = [
    (4, 80, 100),     # G.conv6_1 on the wide halo kernel, 100 % 16 = 4
    (1, 80, 345),     # ... 345 % 16 = 9, one stream; the widest map
    (8, 80, 208),     # G.cb5 (40 x 104) on the wide halo kernel, G.conv6_1 on halo_c32; the Cout = 1 pair fused
    (2, 80, 37),      # odd width: the pair unfused (conv6_2 the plain Cout = 1 kernel), E.conv1 Cin = 1 at odd width and stride 2
    (1, 80, 61),
    (1, 80, 7),
    (1, 80, 1),       # M = 1 at the bottleneck
    (2, 68, 32),      # the inpainter tests' size: odd map heights 17, 9, 5
    (8, 80, 225),     # the smallest 8-stream clip whose G.cb4 (20 x 113, with the virtual concat) runs the wide halo kernel: 20 % 8 = 4
]

Layer = collections.namedtuple("Layer", "name desc M OH OW")     # desc: the 17 fields of Conv2dDesc; M = N * OH * OW

_holders = []


def _generator():
    if not _holders:
        from viai_amd import networks as N
        _holders.extend((N.MelEncoder(), N.MelDecoder()))
    return _holders


def _desc(shape, c2, conv):
    from viai_amd import networks as N
    g = N._conv_geom(conv)
    n, ih, iw, c1 = shape
    return (n, ih, iw, c1, c2, conv.out_channels, g.kernel[0], g.kernel[1], g.stride[0], g.stride[1], g.padding[0], g.padding[1],
            1 if g.transposed else 0, 1, 1, -1, -1)


def generator_layers(B, F, T):
    """[Layer] of MelEncoder + MelDecoder on a (B, F, T) mel, in launch order"""
    from viai_amd import networks as N
    E, G = _generator()
    layers = []

    def run(name, shape, conv, c2=0):
        o = N.out_shape(shape, conv)
        layers.append(Layer(name, _desc(shape, c2, conv), o[0] * o[1] * o[2], o[1], o[2]))
        return o

    x, net = (B, F, T, 1), []
    for i in range(5):
        x = run("E.conv%d" % (i + 1), x, E._modules["conv%d" % (i + 1)])
        net.append(x)
    net[-1] = (x[0], x[1] // 3, x[2], x[3])                                   # ops.avgpool_h(net[-1], 3)
    sizes = [(net[-1 - i][1], net[-1 - i][2]) for i in range(1, len(net))] + [(F, T)]
    out = run("G.deconv1_1", net[-1], G.deconv1_1)
    out = run("G.deconv1_2", out, G.deconv1_2)
    out = (out[0], sizes[0][0], sizes[0][1], out[3])
    for i in range(1, len(net)):
        blk = G._modules["convblock%d" % (i + 1)]
        c2 = net[-(i + 1)][3] if i == G.skip_at else 0
        for j in range(blk.nums):
            out = run("G.cb%d_%d" % (i + 1, j), out, blk._modules["conv%s_%d" % (blk.name, j)], c2 if j == 0 else 0)
        out = (out[0], sizes[i][0], sizes[i][1], out[3])
    out = run("G.conv6_1", out, G.conv6_1)
    run("G.conv6_2", out, G.conv6_2)
    return layers


# ---- the conditions the table as a whole must reach: name -> predicate over (family, desc, M, OH, OW, stat tiles)
def _d(desc):
    return dict(zip(("N", "IH", "IW", "C1", "C2", "Co", "kh", "kw", "sh", "sw", "ph", "pw", "tr"), desc[:13]))


CONDITIONS = collections.OrderedDict([
    ("igemm_sk32x32_f16x2 at M % 32 != 0", lambda f, d, M, OH, OW, t: f == "igemm_sk32x32_f16x2" and M % 32 != 0),
    ("igemm_sk32x32_f16x2 at M < 32", lambda f, d, M, OH, OW, t: f == "igemm_sk32x32_f16x2" and M < 32),
    ("igemm128x32_f16x2 at M % 128 != 0", lambda f, d, M, OH, OW, t: f == "igemm128x32_f16x2" and M % 128 != 0),
    ("igemm128x32_f16x2 with a virtual concat at ragged M", lambda f, d, M, OH, OW, t: f == "igemm128x32_f16x2" and _d(d)["C2"] > 0 and M % 128 != 0),
    ("halo_wide32_f16x2 with (8, 16) tiles clipped on the right", lambda f, d, M, OH, OW, t: f == "halo_wide32_f16x2" and t == (8, 16) and OW % 16 != 0),
    ("halo_wide32_f16x2 with (8, 16) tiles clipped below", lambda f, d, M, OH, OW, t: f == "halo_wide32_f16x2" and t == (8, 16) and OH % 8 != 0),
    ("halo_c32_f16x2", lambda f, d, M, OH, OW, t: f == "halo_c32_f16x2"),
    ("Cin = 1 direct at odd width and stride 2", lambda f, d, M, OH, OW, t: f == "direct" and _d(d)["C1"] + _d(d)["C2"] == 1 and _d(d)["IW"] % 2 == 1 and _d(d)["sw"] == 2),
])


def stat_tiles(lib, desc):
    import ctypes as C
    from viai_amd._lib import Conv2dDesc
    th, tw = C.c_int(), C.c_int()
    lib.viai_conv2d_stat_tiles(C.byref(Conv2dDesc(*desc)), C.byref(th), C.byref(tw))
    return th.value, tw.value


def route(lib, desc, form=1):
    """(family, launches) of the forward of `desc` with fp32 (0) or abs-max (1) operands"""
    import ctypes as C
    from viai_amd._lib import Conv2dDesc
    buf = C.create_string_buffer(64)
    n = lib.viai_conv2d_route(C.byref(Conv2dDesc(*desc)), 0, form, buf, 64)
    return buf.value.decode(), n


def pair_ok(lib, layers):
    """does G.conv6_1 -> conv6_2 run as the fused pair?  (ops.conv_bn_act_cout1_ok's query, without tensors)"""
    import ctypes as C
    from viai_amd._lib import Conv2dDesc
    l61 = [l for l in layers if l.name == "G.conv6_1"][0]
    d2 = (l61.desc[0], l61.OH, l61.OW, l61.desc[5], 0, 1, 3, 3, 1, 1, 1, 1, 0, 1, 1, -1, -1)
    return bool(lib.viai_pair_cout1_ok(C.byref(Conv2dDesc(*d2))))
