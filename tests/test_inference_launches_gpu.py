"""Every conv launch of AudioModel.test() at ragged clip shapes, and the generator as a whole, against fp64.

The timed step (tests/test_step_launches_gpu.py) runs 16 x 256 x 256, where every tile of every kernel is full.  Inference runs clips of any
length with 1 .. 8 streams and eval-mode BatchNorm: almost every tile is clipped, the split-K kernel's last 32-row block is partial (M down to 3
at the bottleneck of a one-frame clip), 128-row tiles straddle two images, the BatchNorm + align-corners resize goes to odd targets, and
avgpool_h sees a 3-row map.  tests/inference_common.py holds the shapes; tests/test_inference_routes_cpu.py holds them to the kernels they
were chosen for.

CENSUS: set_inputs + test() under no_grad at every shape, recorded with run_census of the step-launch test (loaded by path, as it loads its
own neighbours).  Every routed record must have the family and launch count viai_conv2d_route predicts, and the conditions of the CPU test
must occur in the RECORDED families and descriptors.
REPLAY: every distinct viai_conv2d_fwd / _fwd_amax / _fwd_p16 launch again through replay() on fresh operands: `y` and the worst `tile`
against torch fp64 on the CPU, tiles clipped at the map's edge counted as tiles of their own (_worst_tile_clipped).  Bounds: TOL of the
step-launch test, measured there at larger M with the same K.  Beside each launch the table prints the error of torch's fp32 CPU conv on the same
operands: a bound may rise to 3x that, no further (RAISED; empty: no launch needed it).  Measured on the MI355X over the 137 distinct launches:
worst y 3.7e-7 and tile 4.1e-7 (G.cb4_0, 64 + 64 -> 32 on igemm128x32_f16x2; the fp32 CPU conv 5.9e-7 / 6.2e-7 there, 8.3e-7 at its worst),
against bounds of 2e-6 / 2.3e-6; the Cin = 1 / Cout = 1 layers and the pair 9.0e-8 per column at most.
FUSED AND DIRECT LAYERS: E.conv1 (Cin = 1, masked), G.conv6_1 -> conv6_2 as the fused pair, conv6_2 alone, through ops.conv_bn_act /
ops.conv_bn_act_cout1 with training=False at the geometries inference_common derives, error per output column.
COMPLETENESS: a census record that is neither replayed nor at a geometry of the fused-layer test fails as an inference launch without a value
test.
WHOLE NETWORK and STREAMS: see the tests.

VIAI_INFERENCE_PROFILE=path: the census, per-launch errors and whole-network errors are written there as JSON (profiles/inference_launches.json
is such a file).
"""
import importlib.util
import json
import os
import time

import pytest
import torch
import torch.nn.functional as F

import inference_common as IC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = IC.INFERENCE_SHAPES
STREAM_SHAPES = [(2, 80, 37), (8, 80, 37), (2, 80, 208), (8, 80, 208)]
PROFILE = {"census": {}, "launches": [], "layers": [], "network": {}, "streams": {}}

# (entry, desc) -> {"y": bound, "tile": bound}: launches whose bound had to rise above TOL, each at most 3x the fp32 CPU conv's error on the same
# operands, with the measured values.  None did.
RAISED = {}


def _load(name):
    spec = importlib.util.spec_from_file_location("_inference_" + name, os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


SL = _load("test_step_launches_gpu")


def _sid(shape):
    return "%dx%dx%d" % tuple(shape)


def _dump():
    path = os.environ.get("VIAI_INFERENCE_PROFILE")
    if path:
        with open(path, "w") as f:
            json.dump(PROFILE, f, indent=1, sort_keys=True)


class _Threads:
    """torch's CPU threads at most 16 during the fp64 work (as replay_all)"""

    def __enter__(self):
        self.n = torch.get_num_threads()
        torch.set_num_threads(min(16, self.n))

    def __exit__(self, *a):
        torch.set_num_threads(self.n)


# ---------------------------------------------------------------------------------------------------------------------------- inputs
def _states():
    """oracle states with running statistics that matter: means in +-0.2, variances in 0.5 .. 1.5 (tests/test_networks_gpu.py
    test_eval_mode_uses_running_stats)"""
    from oracle import viai_oracle as O
    out = []
    for nm, sd in (("E", O.encoder_state()), ("G", O.decoder_state())):
        for k in sd:
            if k.endswith("running_var"):
                sd[k] = O.cf_uniform("inf.%s.%s" % (nm, k), tuple(sd[k].shape), 0.5, 1.5)
            if k.endswith("running_mean"):
                sd[k] = O.cf_uniform("inf.%s.%s" % (nm, k), tuple(sd[k].shape), -0.2, 0.2)
        out.append(sd)
    return out


def _inputs(shape):
    """(s (B, 1, F, T) in [0, 1], mask (B, 1, 1, T)): one gap of max(T / 4, 1) frames per clip; clip 0's gap ends at the last frame, the others'
    lie where oracle.make_mask puts them.  A one-frame clip keeps its frame (a gap would leave the generator nothing but zeros)."""
    from oracle import viai_oracle as O
    B, Fb, T = shape
    s = O.cf_uniform("inf.s.%d.%d.%d" % shape, (B, 1, Fb, T))
    mask = O.make_mask(B, T, "inf.mask.%d.%d.%d" % shape) if T > 1 else torch.ones(B, 1, 1, T)
    if T > 1:
        L = max(T // 4, 1)
        mask[0] = 1.0
        mask[0, :, :, T - L:] = 0.0
        assert all(0 < float(mask[b].sum()) < T for b in range(B)) and float(mask[0, 0, 0, -1]) == 0.0
    return s, mask


@pytest.fixture(scope="module")
def model():
    from oracle import viai_oracle as O
    from viai_amd.model import AudioModel, StepConfig
    hp = StepConfig()
    hp.cin_channels, hp.max_mel_lengths = 80, 256
    m = AudioModel(hp, device="cuda")
    sdE, sdG = _states()
    m.load_states(sdE, sdG, O.disc_state())
    m.train = 0
    yield m
    m.close()
    del m
    torch.cuda.empty_cache()


def _run_test(model, s, mask):
    model.set_inputs(s, mask)
    with torch.no_grad():
        return model.test()


# ---------------------------------------------------------------------------------------------------------------------------- census
@pytest.fixture(scope="module")
def census(model):
    t0 = time.time()
    c = {}
    for shape in SHAPES:
        s, mask = _inputs(shape)
        c[shape] = SL.run_census(model, run=lambda i: _run_test(model, s, mask))
        PROFILE["census"][_sid(shape)] = c[shape]
    print("\ninference census: %s distinct launches in %.1f s" % (" + ".join(str(len(c[k])) for k in SHAPES), time.time() - t0))
    for shape in SHAPES:
        for r in sorted(c[shape], key=lambda r: (r["entry"], r["desc"])):
            print("  %-10s %-26s %-40s %-24s %s x%d" % (_sid(shape), r["entry"][5:], SL._Geom(tuple(r["desc"])).short(), r["family"],
                                                      " ".join("%s=%d" % kv for kv in sorted(r["opts"].items()) if kv[1]), r["count"]))
    _dump()
    return c


def _fused_geoms(shape):
    """the geometries the fused-layer test runs at a shape, derived on the host: {(kind, key)}"""
    from viai_amd import _lib
    layers = {l.name: l for l in IC.generator_layers(*shape)}
    B, Fb, T = shape
    out = {("cin1", layers["E.conv1"].desc)}
    if IC.pair_ok(_lib.load(), list(layers.values())):
        out.add(("pair", (B, Fb, T, 32)))
    else:
        out.add(("cout1", layers["G.conv6_2"].desc))
    return out


def _covered_by_fused(shape, rec):
    d = tuple(rec["desc"])
    geoms = _fused_geoms(shape)
    if rec["entry"].startswith("viai_pair_cout1"):
        return ("pair", (d[0], d[1], d[2], d[3])) in geoms
    return False


def test_census_matches_the_routes_and_reaches_the_conditions(census):
    from viai_amd import _lib, ops
    lib = _lib.load()
    reached = set()
    for shape in SHAPES:
        recs = census[shape]
        routed = [r for r in recs if r["entry"] in SL.ROUTE_OF]
        assert len(routed) >= 14, (shape, len(routed))
        assert all(r["entry"] == "viai_conv2d_fwd_amax" for r in routed), sorted({r["entry"] for r in routed})      # eval never pre-splits
        off = ["%s %s: launched %s x%d, route %s x%d" % ((r["entry"], SL._Geom(tuple(r["desc"])).short(), r["family"], r["launches"]) + SL._route(lib, r))
               for r in routed if SL._route(lib, r) != (r["family"], r["launches"])]
        assert not off, "%s: viai_conv2d_route disagrees with the launch:\n  " % (shape,) + "\n  ".join(off)
        # every layer the host walk derives was launched, and nothing else
        want = {l.desc for l in IC.generator_layers(*shape)}
        pair = any(r["entry"] == "viai_pair_cout1_fwd" for r in recs)
        if pair:
            want = {d for d in want if d[5] != 1}
        assert {tuple(r["desc"]) for r in routed} == want, shape
        reached.add("pair" if pair else "no pair")
        assert pair != any(r["desc"][5] == 1 for r in routed), shape
        for r in routed:
            g = SL._Geom(tuple(r["desc"]))
            tiles = ops.conv_desc(*r["desc"])["tiles"]
            reached.update(n for n, cond in IC.CONDITIONS.items() if cond(r["family"], tuple(r["desc"]), g.N * g.OH * g.OW, g.OH, g.OW, tiles))
    want = set(IC.CONDITIONS) | {"pair", "no pair"}
    assert reached == want, "not in the census: %s" % sorted(want - reached)


def test_every_inference_launch_has_a_value_test(census):
    missing = []
    for shape in SHAPES:
        checked = {tuple(r["desc"]) for r in census[shape] if SL._replayable(r)}
        for kind, key in _fused_geoms(shape):
            if kind != "pair":
                checked.add(tuple(key))
            else:
                l61 = [l for l in IC.generator_layers(*shape) if l.name in ("G.conv6_1", "G.conv6_2")]
                checked.update(l.desc for l in l61)
        for r in census[shape]:
            if SL._replayable(r) or _covered_by_fused(shape, r):
                continue
            if r["entry"] in SL.PACKS and tuple(r["desc"]) in checked:          # packed at a descriptor a checked launch packs at
                continue
            missing.append("%s: %s %s [%s]" % (_sid(shape), r["entry"], SL._Geom(tuple(r["desc"])).short(), r["family"]))
    assert not missing, "inference launch without a value test:\n  " + "\n  ".join(sorted(set(missing)))


# ---------------------------------------------------------------------------------------------------------------------------- replay
def _worst_tile_clipped(a, b, th=8, tw=16):
    """largest relative error of any th x tw output tile of an NCHW tensor, the ragged last tile rows and columns as tiles of their own
    (equal to _worst_tile of the step-launch test where the map divides evenly)"""
    N, Cc, H, W = a.shape
    ph, pw = -H % th, -W % tw
    d = F.pad((a - b).pow(2).sum(1), (0, pw, 0, ph)).reshape(N, (H + ph) // th, th, (W + pw) // tw, tw).sum(dim=(2, 4))
    r = F.pad(b.pow(2).sum(1), (0, pw, 0, ph)).reshape(N, (H + ph) // th, th, (W + pw) // tw, tw).sum(dim=(2, 4))
    return float((d / (r + 1e-300)).sqrt().max())


def test_the_clipped_tile_error_sees_a_clipped_tile():
    """host only: equal to _worst_tile on full tiles; an error confined to the last, 1-column tile is seen at its own size"""
    g = torch.Generator().manual_seed(1)
    b = torch.randn(2, 4, 16, 32, generator=g, dtype=torch.float64)
    a = b + 1e-6 * torch.randn(b.shape, generator=g, dtype=torch.float64)
    assert abs(_worst_tile_clipped(a, b) - SL._worst_tile(a, b)) < 1e-18
    b = torch.randn(1, 4, 20, 33, generator=g, dtype=torch.float64)
    a = b.clone()
    a[:, :, 16:, 32] *= 1.5
    assert abs(_worst_tile_clipped(a, b) - 0.5) < 1e-12 and SL._worst_tile(a, b) < 0.05


def _first_shape(census, rec):
    key = (rec["entry"], tuple(rec["desc"]), rec["family"], tuple(sorted(rec["opts"].items())))
    for shape in SHAPES:
        for r in census[shape]:
            if (r["entry"], tuple(r["desc"]), r["family"], tuple(sorted(r["opts"].items()))) == key:
                return shape


@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_inference_launches_against_fp64(census, shape):
    """every distinct forward launch of test() at this shape (those an earlier shape of the table made already are replayed there)"""
    recs = [r for r in census[shape] if SL._replayable(r) and _first_shape(census, r) == shape]
    assert all(r["entry"].startswith("viai_conv2d_fwd") for r in recs)
    gen = torch.Generator(device="cuda").manual_seed(20261021)
    rows, bad = [], []
    t00 = time.time()
    print("\nreplay of the launches of test() at %s against fp64 (o32: torch's fp32 CPU conv on the same operands):" % _sid(shape))
    with _Threads():
        for rec in sorted(recs, key=lambda r: (r["entry"], r["desc"])):
            g = SL._Geom(tuple(rec["desc"]))
            t0 = time.time()
            keep, msg = {}, None
            try:
                seen, errs = SL.replay(rec, gen, worst_tile=_worst_tile_clipped, keep=keep)
                y32 = SL._act64((g.fwd64(keep["x"].float(), keep["w"].float()) + (keep["bias"].float().view(1, -1, 1, 1) if keep["bias"] is not None else 0)).double(),
                                keep["act"])
                o32 = {"y": SL._relerr(y32, keep["truth"]), "tile": _worst_tile_clipped(y32, keep["truth"])}
                if seen != rec["family"]:
                    msg = "family %s, test() ran %s" % (seen, rec["family"])
                bound = dict(SL.TOL, **RAISED.get((rec["entry"], tuple(rec["desc"])), {}))
                over = [k for k, v in errs.items() if not v <= bound[k]]
                if over:
                    msg = (msg + "; " if msg else "") + "over the bound: " + ", ".join(over)
            except Exception as e:          # (a library error is a finding of this launch: report it with the others)
                seen, errs, o32, msg = "?", {}, {}, "%s: %s" % (type(e).__name__, e)
            opt = " ".join("%s=%d" % (k, v) for k, v in sorted(rec["opts"].items()) if v)
            row = "%-26s %-40s %-24s %-28s %s | o32 %s  (%.1fs)" % (rec["entry"][12:], g.short(), rec["family"], opt,
                                                                  " ".join("%s %.2e" % kv for kv in sorted(errs.items())),
                                                                  " ".join("%s %.2e" % kv for kv in sorted(o32.items())), time.time() - t0)
            rows.append(row)
            print(("FAIL " if msg else "ok   ") + row + ("  <-- " + msg if msg else ""))
            PROFILE["launches"].append({"shape": _sid(shape), "entry": rec["entry"], "desc": rec["desc"], "family": rec["family"], "opts": rec["opts"],
                                        "hip": errs, "o32": o32})
            if msg:
                bad.append("%s %s [%s]: %s" % (rec["entry"], g.short(), rec["family"], msg))
            torch.cuda.empty_cache()
    print("%d launches in %.1f s" % (len(rows), time.time() - t00))
    _dump()
    assert rows or shape != SHAPES[0]
    assert not bad, "%d of %d launches of test() at %s off:\n  " % (len(bad), len(rows), _sid(shape)) + "\n  ".join(bad)


# ---------------------------------------------------------------------------------------------------------------------------- fused and direct layers
def _col_errs(a, b):
    """(whole-tensor relative error, worst relative error of one time column of one clip) of NCHW tensors"""
    a, b = a.double().cpu(), b.double().cpu()
    d = (a - b).pow(2).sum(dim=(1, 2)).sqrt()
    r = b.pow(2).sum(dim=(1, 2)).sqrt()
    return ((a - b).norm() / (b.norm() + 1e-300)).item(), float((d / (r + 1e-300)).max())


def _bn_holder(c, tag):
    from oracle import viai_oracle as O
    bn = torch.nn.BatchNorm2d(c)
    with torch.no_grad():
        bn.weight.copy_(O.cf_uniform(tag + ".g", (c,), 0.5, 1.5))
        bn.bias.copy_(O.cf_uniform(tag + ".b", (c,), -0.3, 0.3))
        bn.running_mean.copy_(O.cf_uniform(tag + ".m", (c,), -0.2, 0.2))
        bn.running_var.copy_(O.cf_uniform(tag + ".v", (c,), 0.5, 1.5))
    return bn.cuda().eval()


def _bn64(bn, y, fp=torch.float64):
    sc = bn.weight.detach().cpu().to(fp) * torch.rsqrt(bn.running_var.cpu().to(fp) + bn.eps)
    return (y - bn.running_mean.cpu().to(fp).view(1, -1, 1, 1)) * sc.view(1, -1, 1, 1) + bn.bias.detach().cpu().to(fp).view(1, -1, 1, 1)


# Per column of the fused / direct layers: the project's own bounds for one conv (TOL y whole tensor, TOL tile for the smallest unit looked at)
LAYER_TOL = {"y": SL.TOL["y"], "col": SL.TOL["tile"]}


@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_fused_and_direct_layers_in_eval_mode_per_column(census, shape):
    """E.conv1 with the mask (Cin = 1, eval: mask_mul + the streaming kernel), and the decoder's tail: the fused Cout = 1 pair where the census shows
    it, conv6_2 alone on the plain Cout = 1 kernel where not.  fp64 truth; the error of every output column of every clip on its own, so one confined
    to the last column (which reads only padding on the right at odd T) or the last frame cannot hide."""
    from oracle import viai_oracle as O
    from viai_amd import ops
    B, Fb, T = shape
    recs = census[shape]
    geoms = _fused_geoms(shape)
    tag = "inf.layer.%s" % _sid(shape)
    _, mask = _inputs(shape)
    out = {}

    def both(fn, *ts):
        """fn on fp64 and on fp32 CPU tensors"""
        return fn(torch.float64, *[t.detach().double().cpu() for t in ts]), fn(torch.float32, *[t.detach().float().cpu() for t in ts]).double()

    with _Threads(), torch.no_grad():
        # ---- E.conv1
        (d1,) = [k for kind, k in geoms if kind == "cin1"]
        assert any(tuple(r["desc"]) == d1 and r["entry"] == "viai_conv2d_fwd_amax" and r["family"] == "direct" for r in recs), "the census has no such E.conv1"
        x = O.cf_uniform(tag + ".x", (B, Fb, T, 1), -1, 1).cuda()
        w = O.cf_std(tag + ".w1", (32, 1, 3, 3), 1 / 3.0).cuda()
        bn = _bn_holder(32, tag + ".bn1")
        z = ops.conv_bn_act(x, w, None, bn, kernel=(3, 3), stride=(2, 2), padding=(1, 1), act=ops.ACT_LRELU, training=False, xmask=mask.cuda())
        t64, t32 = both(lambda fp, x_, w_: F.leaky_relu(_bn64(bn, F.conv2d((x_.permute(0, 3, 1, 2) * mask.to(fp)), w_, None, (2, 2), (1, 1)), fp), 0.2), x, w)
        out["E.conv1"] = (_col_errs(z.permute(0, 3, 1, 2), t64), _col_errs(t32, t64))
        # ---- the decoder's tail
        xin = O.cf_uniform(tag + ".x6", (B, Fb, T, 32), -1, 1).cuda()
        w2 = O.cf_std(tag + ".w62", (32, 1, 3, 3), 1 / 17.0).cuda()
        b2 = O.cf_uniform(tag + ".b62", (1,), -0.1, 0.1).cuda()
        if ("pair", (B, Fb, T, 32)) in geoms:
            assert any(r["entry"] == "viai_pair_cout1_fwd" and tuple(r["desc"][:4]) == (B, Fb, T, 32) for r in recs), "the census has no such pair"
            w61 = O.cf_std(tag + ".w61", (32, 32, 3, 3), 1 / 17.0).cuda()
            b61 = O.cf_uniform(tag + ".b61", (32,), -0.1, 0.1).cuda()
            bn6 = _bn_holder(32, tag + ".bn6")
            p = ops.conv_bn_act_cout1(xin, w61, b61, bn6, w2, b2, kernel=(3, 3), stride=(1, 1), padding=(1, 1), transposed=True, act=ops.ACT_RELU,
                                      transposed2=True, act2=ops.ACT_SIGMOID, training=False)
            t64, t32 = both(lambda fp, x_, wa, ba, wb, bb: torch.sigmoid(F.conv_transpose2d(
                F.relu(_bn64(bn6, F.conv_transpose2d(x_.permute(0, 3, 1, 2), wa, ba, 1, 1), fp)), wb, bb, 1, 1)), xin, w61, b61, w2, b2)
            out["G.conv6_1 -> conv6_2 (pair)"] = (_col_errs(p.permute(0, 3, 1, 2), t64), _col_errs(t32, t64))
        else:
            (d2,) = [k for kind, k in geoms if kind == "cout1"]
            assert any(tuple(r["desc"]) == d2 and r["family"] == "direct" and r["opts"]["act"] == ops.ACT_SIGMOID for r in recs), "the census has no such conv6_2"
            p = ops.conv_bn_act(xin, w2, b2, None, kernel=(3, 3), stride=(1, 1), padding=(1, 1), transposed=True, act=ops.ACT_SIGMOID, training=False)
            t64, t32 = both(lambda fp, x_, wb, bb: torch.sigmoid(F.conv_transpose2d(x_.permute(0, 3, 1, 2), wb, bb, 1, 1)), xin, w2, b2)
            out["G.conv6_2 (Cout = 1)"] = (_col_errs(p.permute(0, 3, 1, 2), t64), _col_errs(t32, t64))
    bad = []
    for name, ((ey, ecol), (oy, ocol)) in out.items():
        print("%-10s %-30s y %.2e col %.2e | o32 y %.2e col %.2e" % (_sid(shape), name, ey, ecol, oy, ocol))
        PROFILE["layers"].append({"shape": _sid(shape), "layer": name, "hip": {"y": ey, "col": ecol}, "o32": {"y": oy, "col": ocol}})
        if not (ey <= LAYER_TOL["y"] and ecol <= LAYER_TOL["col"]):
            bad.append((name, ey, ecol))
    _dump()
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------------- whole network
_BLOCK_NUMS = {2: 3, 3: 3, 4: 3, 5: 4}


def _generator64(sdE, sdG, x, fp=torch.float64):
    """MelEncoder + MelDecoder in eval mode with torch.nn.functional alone, in `fp` -- the oracle's layers restated: its bilinear_ac
    rounds the interpolation weights to fp32.  x: (B, 1, F, T), already masked.  -> [5 encoder maps (the last one pooled), the output]"""
    E = {k: v.to(fp) for k, v in sdE.items() if v.is_floating_point()}
    G = {k: v.to(fp) for k, v in sdG.items() if v.is_floating_point()}

    def bn(sd, p, y):
        sc = sd[p + ".weight"] * torch.rsqrt(sd[p + ".running_var"] + 1e-5)
        return (y - sd[p + ".running_mean"].view(1, -1, 1, 1)) * sc.view(1, -1, 1, 1) + sd[p + ".bias"].view(1, -1, 1, 1)

    def ct(name, y, pad):
        return F.relu(bn(G, name + "_bn", F.conv_transpose2d(y, G[name + ".weight"], G.get(name + ".bias"), 1, pad)))

    x = x.to(fp)
    hw = tuple(x.shape[2:])
    net = []
    for i, stride in enumerate(((2, 2), (2, 1), (2, 2), (2, 2), (2, 2))):
        x = F.leaky_relu(bn(E, "bn%d" % (i + 1), F.conv2d(x, E["conv%d.weight" % (i + 1)], None, stride, (1, 1))), 0.2)
        net.append(x)
    net[-1] = F.avg_pool2d(net[-1], (3, 1))
    out = ct("deconv1_2", ct("deconv1_1", net[-1], (0, 1)), (1, 1))
    for i in range(1, 5):
        out = F.interpolate(out, size=tuple(net[-1 - i].shape[2:]), mode="bilinear", align_corners=True)
        if i == 3:
            out = torch.cat((out, net[-(i + 1)]), 1)
        for j in range(_BLOCK_NUMS[i + 1]):
            out = ct("convblock%d.conv%d_%d" % (i + 1, i + 1, j), out, (1, 1))
    out = F.interpolate(out, size=hw, mode="bilinear", align_corners=True)
    out = ct("conv6_1", out, (1, 1))
    return net + [torch.sigmoid(F.conv_transpose2d(out, G["conv6_2.weight"], G["conv6_2.bias"], 1, 1))]


_REF = {}
MAPS = ("e1", "e2", "e3", "e4", "e5", "fake")


def _reference(shape):
    """(s, mask, fp64 maps, the fp32 CPU oracle's maps) at a shape, computed once"""
    if shape not in _REF:
        from oracle import viai_oracle as O
        s, mask = _inputs(shape)
        sdE, sdG = _states()
        with _Threads(), torch.no_grad():
            t64 = _generator64(sdE, sdG, s * mask)
            fe = O.encoder_forward(sdE, (s * mask).reshape(shape), training=False)
            o32 = list(fe) + [O.decoder_forward(sdG, fe, s.shape, training=False)]
        _REF[shape] = (s, mask, t64, [t.double() for t in o32])
    return _REF[shape]


def _hip_maps(model, s, mask):
    """the five encoder maps (eval mode, as test() runs them) and test()'s output, NCHW on the host"""
    fake = _run_test(model, s, mask).detach().double().cpu()
    B, _, Fb, T = s.shape
    was = model.Mel_Encoder.training
    model.Mel_Encoder.eval()
    try:
        with torch.no_grad():
            feats = model.Mel_Encoder.forward_nhwc(model.mel.view(B, Fb, T), mask=model.mask)
    finally:
        model.Mel_Encoder.train(was)
    return [f.permute(0, 3, 1, 2).detach().double().cpu() for f in feats] + [fake]


def _network_bad(tag, hip, t64, o32, report):
    bad = []
    for name, h, t, o in zip(MAPS, hip, t64, o32):
        assert tuple(h.shape) == tuple(t.shape) == tuple(o.shape), (name, h.shape, t.shape, o.shape)
        (ey, ecol), (oy, ocol) = _col_errs(h, t), _col_errs(o, t)
        report[name] = {"hip": {"y": ey, "col": ecol}, "o32": {"y": oy, "col": ocol}}
        print("%-12s %-5s hip y %.2e col %.2e | o32 y %.2e col %.2e" % (tag, name, ey, ecol, oy, ocol))
        if not (ey <= 3 * oy and ecol <= 3 * ocol):
            bad.append((name, ey, ecol, oy, ocol))
    return bad


@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_generator_in_eval_mode_against_fp64(model, shape):
    """test() against the generator evaluated in fp64 (states and input cast to double, every layer with torch.nn.functional): the five encoder
    maps and the output, whole-tensor relative error and the worst relative error of one time column of one clip.  This is what covers the passes
    between the convs at odd sizes: eval coefficients, the fused BatchNorm + resize to odd targets, bilinear_ac on its own, avgpool_h on a 3-row map,
    the mask on the Cin = 1 load.  Bound: 3x the error of the fp32 CPU oracle (oracle.viai_oracle in eval mode) against the same fp64 truth at the
    same shape, quantity by quantity.  Measured (profiles/inference_launches.json): the encoder maps 7.1e-8 .. 1.9e-7 where the oracle has 7.1e-8 ..
    2.5e-7; the output at worst 3.0e-7 in one column (8 x 80 x 208; oracle 4.9e-7); the largest ratio to the oracle's error 1.47 (2 x 68 x 32, output,
    one column: 2.8e-7 against 1.9e-7), 1.84 over the single clips of the stream test -- no bound had to rise."""
    s, mask, t64, o32 = _reference(shape)
    hip = _hip_maps(model, s, mask)
    rep = PROFILE["network"][_sid(shape)] = {}
    bad = _network_bad(_sid(shape), hip, t64, o32, rep)
    _dump()
    assert not bad, bad


@pytest.mark.parametrize("shape", STREAM_SHAPES, ids=_sid)
def test_a_clip_alone_and_in_a_batch(model, shape):
    """clip b of a batch of B against the same clip run alone (eval mode: the truth of a clip does not depend on its neighbours).  Not bitwise: M
    changes the route.  Both runs within the whole-network bound of the fp64 truth, column by column -- a 32- or 128-row tile that straddles two
    images and takes its rows from the wrong one fails here."""
    s, mask, t64, o32 = _reference(shape)
    B = shape[0]
    hip = _hip_maps(model, s, mask)
    rep = PROFILE["streams"][_sid(shape)] = {}
    bad = _network_bad(_sid(shape) + " batch", hip, t64, o32, rep.setdefault("batch", {}))
    for b in range(B):
        alone = _hip_maps(model, s[b:b + 1], mask[b:b + 1])
        bad += [(b,) + x for x in _network_bad("%s clip %d" % (_sid(shape), b), alone, [t[b:b + 1] for t in t64], [o[b:b + 1] for o in o32],
                                               rep.setdefault("clip%d" % b, {}))]
    _dump()
    assert not bad, bad
