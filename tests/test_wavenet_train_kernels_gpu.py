"""The kernels of a teacher-forced WaveNet training step, each called at the C ABI and compared with torch in fp64 on the CPU (autograd for
the backward passes) on the same fp32 inputs.  (Dropout, the masked cross-entropy and the class embedding have their own files.)

A. CONV1D LAUNCHES.  conv1d_apply -> ops.conv_bn_act runs a layer without BatchNorm as: forward `viai_conv2d_fwd_amax` (x_amax given where
viai_conv2d_fwd_f16_ok says the kernel splits its activations, NULL otherwise; ops._stage_input / _conv_fwd), backward with no abs-max of dy
(ops._ConvBnAct.backward: want_amax stays False without a BatchNorm), so `viai_conv2d_dgrad` on the `viai_conv2d_pack_dgrad` image and
`viai_conv2d_wgrad` -- route forms AMAX / F32 / F32.  For every layer kind the family of each pass is asked on the host at N = 2, IW = 8192
(viai_conv2d_route); the test length is the smallest T of 64, 128, ... with the same three families, then T + 5 (M no multiple of any tile;
compared with the route at 8192 + 5) and T = 40.  After every launch viai_conv2d_last_kernel must name the predicted family.

Families reached on the MI355X (N = 2; fwd / dgrad / wgrad; ksplit of the weight gradient from viai_conv2d_wgrad_ws_bytes):
  512->512 k3 d32        T 8192, 8197: igemm128x256_f16x2 / igemm128x128_bf16x3 / wgrad_bf3_bf16x3      T 40: igemm_sk32x32_f16x2 / igemm_sk32x32_bf16x3 / wgrad_bf3_bf16x3
  80->512, 256->512      T 8192, 8197: igemm128x256_f16x2 / igemm64x64_bf16x3 / wgrad_bf3_bf16x3        T 40: both split-K, wgrad_bf3_bf16x3
  256->256 (skip, head)  T 4096, 4101: igemm64x64_f16x2 / igemm64x64_bf16x3 / wgrad_bf3_bf16x3          T 40: both split-K, wgrad_bf3_bf16x3
  256->32 (head, padded) T 4096, 4101: igemm128x32_f16x2 / igemm64x64_bf16x3 / wgrad_mfma_f32           T 40: igemm128x32_f16x2 / igemm_sk32x32_bf16x3 / wgrad_mfma_f32
  64->64 k3 (all d)      every T: igemm_sk32x32_f16x2 / igemm_sk32x32_bf16x3 / wgrad_bf3_bf16x3 -- at 64 channels the split-K kernel IS the training route
  80->64                 T 8192, 8197: igemm_sk32x32_f16x2 / igemm64x64_bf16x3 / wgrad_bf3_bf16x3       T 40: dgrad split-K
  32->64                 igemm_sk32x32_f16x2 / igemm128x32_bf16x3 / wgrad_mfma_f32
  32->32, 16->32 1x1     igemm128x32_f16x2 / igemm128x32_bf16x3 / wgrad32_all_taps_f32 where T % 32 == 0, wgrad_mfma_f32 otherwise
  32->32 k3              as above; wgrad32_all_taps_f32 only at d = 1 (tap span 2), wgrad_mfma_f32 at d >= 2
  80->32                 T 8192, 8197: igemm128x32_f16x2 / igemm64x64_bf16x3 / wgrad_mfma_f32           T 40: dgrad split-K
So each of forward and data gradient runs split-K and plain kernels; the weight-gradient families carry their split count inside
(test_conv_cases_cover_both_sides_of_every_switch derives it: 1 and > 1 both occur).

The 30-channel output layer: WaveNet.forward_nhwc pads its weight to 32 rows, so the step runs Cout = 32 (above).  An UNPADDED Cout = 30 has
a forward route only; the library refuses its data and weight gradient on the host (route_dgrad: Cout % 16 != 0 leaves the exact-fp32 igemm,
which takes contraction lengths in fours only -- 30 is not).  There is therefore no fp32 data-gradient launch of that layer to test;
test_unpadded_output_layer_has_no_backward pins the refusal, and the padded form is compared with the 30-channel fp64 layer.

Bounds: tests/test_step_launches_gpu.py TOL (y, dx 2e-6; dw, db 3e-6 Frobenius-relative), unchanged, on every case; its adjointness bound 7.5e-10 of
|y| |gy| from 2^21 output elements on, scaled by sqrt(2^21 / n) below (adj_bound: the figure of independent output errors goes like 1 / sqrt(n)).

B. NON-CONV KERNELS (csrc/wavenet_ops.hip), one row per launch branch:
  weight_norm_fwd / _bwd     L = 1, L = 256 (one stride), 192 (< one stride), 576 and 1537 (loop, with remainder); accumulate 0 / 1   test_weight_norm
  glu_fwd / _bwd             yc NULL / set; H / 4 = 1, 8, 64; rows * H / 4 > 8192 * 256 (grid wraps)                                    test_glu, test_glu_grid_cap
  outer_fwd, outer_bwd_*     C / 4 = 16, 24 (256 / 24: 16 idle lanes), 512 (two group passes); one row, one block, four ragged blocks   test_outer
  upsample_fwd / _bwd_*      KH 1 / 3; S 4, 5, 16 (S < 16 lanes); F = 1 (no neighbour row), T = 3 .. 300; dx NULL / set; accumulate     test_upsample
  mol_loss, masked_mean      mask NULL / ones / whole zero rows; dyhat NULL; pitch 32 / 40; rows 77, 300, 1000 (no multiple of 256)     test_mol_loss
                             (rows > 8192 * 256 left out: 268 MB of rows and an fp64 mixture over 21 M components take far more than a few seconds)
  relu_fwd, add_scale(b = NULL), scale_by_scalar   n = 4 and past the 8192-block cap, bit for bit                                     test_elementwise_bitwise
Bound of every measured output: 4 x the error of the SAME formula evaluated by torch in fp32 on the CPU against the fp64 truth, same inputs,
same measure (max |err| / max |truth| for elementwise outputs, Frobenius-relative for reductions).  Every figure is printed beside its
yardstick before the assertion (WaveNet section, holds the table measured on the MI355X).
"""
import ctypes as C
import importlib.util
import math
import os

import pytest
import torch
import torch.nn.functional as F

from passes_common import INVALID, assert_bitwise, host, lib, ok, ptr, st
from test_step_launches_gpu import TOL, _relerr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 4.0
EPS32 = 2.0 ** -23
FORM_F32, FORM_AMAX = 0, 1
ACT_NONE, ACT_RELU = 0, 1
# The adjointness figure |<y, gy> - <x, dx>| / (|y| |gy|) of kernels whose outputs carry independent relative errors eps is eps / sqrt(n) for n
# output elements: the errors average out in the inner product.  TOL["adj"] = 7.5e-10 was measured where tests/test_step_launches_gpu.py applies
# the check, on whole batches of 1024 frames (n >= 3.2 M output elements).  Growth law for smaller tensors at the same eps: the bound is
# TOL["adj"] sqrt(2^21 / n) below n = N T Cout = 2^21 and the plain TOL["adj"] from there on (2^21: the 256-channel layers at their training length,
# the smallest tensors of the order the bound was measured at).  At n = 2560 (N = 2, T = 40, 32 channels) that is 2.1e-8.
ADJ_FULL_ELEMENTS = 1 << 21


def adj_bound(n):
    return TOL["adj"] * max(1.0, (ADJ_FULL_ELEMENTS / n) ** 0.5)


N_STEP, T_STEP = 2, 8192                 # the descriptor the routes are asked at: a training batch of the reference-size network


def _tool():
    spec = importlib.util.spec_from_file_location("_conv_routes_tool", os.path.join(ROOT, "tools", "conv_routes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TOOL = _tool()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _uni(g, shape, lo=-1.0, hi=1.0):
    return torch.rand(shape, generator=g, dtype=torch.float32) * (hi - lo) + lo


def _cuda(t):
    return t.detach().to(torch.float32).contiguous().cuda()


def _nan(shape):
    return torch.full(shape, float("nan"), device="cuda")


# ------------------------------------------------------------------------------------------------------------------ the two error measures
def _measure(got, ref64, kind):
    d = host(got).double().reshape(ref64.shape) - ref64
    if kind == "abs":
        return float(d.abs().max() / ref64.abs().max())
    return float(d.norm() / ref64.norm())


def check(got, ref64, f32, what, kind, floor_ulps=0.0):
    """error of `got` against the fp64 truth under MARGIN x the error of the fp32 restatement, same measure; prints both first.
    floor_ulps: only for a named case whose fp32 restatement is exact (see test_upsample)"""
    err, yard = _measure(got, ref64, kind), _measure(f32, ref64, kind)
    print("%-58s %s err %.3e  fp32 torch %.3e  ratio %.2f" % (what, kind, err, yard, err / yard if yard > 0 else (0.0 if err == 0 else float("inf"))))
    assert err <= max(MARGIN * yard, floor_ulps * EPS32), (what, err, yard)
    return err, yard


# ============================================================================================================== A. the Conv1d launches
def _route(desc, p, form):
    L = lib()
    from viai_amd._lib import Conv2dDesc
    buf = C.create_string_buffer(64)
    c = Conv2dDesc(*desc)
    n = L.viai_conv2d_route(C.byref(c), p, form, buf, 64)
    return n, buf.value.decode()


def _fwd_form(desc):
    from viai_amd._lib import Conv2dDesc
    c = Conv2dDesc(*desc)
    return FORM_AMAX if lib().viai_conv2d_fwd_f16_ok(C.byref(c)) else FORM_F32


def step_routes(desc):
    """((launches, family) of forward, data gradient, weight gradient) in the forms the training step uses for a layer without BatchNorm"""
    return tuple(_route(desc, p, f) for p, f in ((0, _fwd_form(desc)), (1, FORM_F32), (2, FORM_F32)))


def wgrad_ksplit(desc):
    """split count of the weight gradient, from the public queries: the workspace is ksplit weight images plus the bias gradient's column-sum partials"""
    from viai_amd import ops
    L = lib()
    d = ops.conv_desc(*desc)
    M = desc[0] * d["OH"] * d["OW"]
    return (d["ws_floats"] - L.viai_colsum_blocks(M, desc[5]) * desc[5]) // d["packed"]


def length_and_routes(cin, cout, k, d, causal, which):
    """(T, the routes predicted for it): "train" the smallest of 64, 128, ... with the families of T_STEP; "ragged" that + 5, whose routes must be
    those of T_STEP + 5; "sk" 40"""
    def at(T):
        return step_routes(TOOL.wavenet_desc(N_STEP, T, cin, cout, k, d, causal))
    want = at(T_STEP)
    T = 64
    while at(T) != want:
        T *= 2
        assert T <= T_STEP
    if which == "train":
        return T, want
    if which == "ragged":
        ragged = at(T_STEP + 5)
        assert ragged[:2] == want[:2], "forward / data gradient change family with a ragged length: %s -> %s" % (want, ragged)
        assert at(T + 5) == ragged, "T = %d: %s, T = %d: %s" % (T + 5, at(T + 5), T_STEP + 5, ragged)
        return T + 5, ragged
    return 40, at(40)


def _conv_truth(x, w, b, gy, k, d, pl, pr, act):
    """fp64 on the CPU: y = act(conv1d(pad(x), w, dilation = d) + b) and the gradients of <y, gy>; x (N, T, Cin), gy (N, T, Cout) channels last"""
    x64 = x.double().permute(0, 2, 1).contiguous().requires_grad_(True)
    w64, b64 = w.double().requires_grad_(True), b.double().requires_grad_(True)
    y = F.conv1d(F.pad(x64, (pl, pr)), w64, b64, dilation=d)
    y = torch.relu(y) if act == ACT_RELU else y
    y.backward(gy.double().permute(0, 2, 1))
    ypre = F.conv1d(F.pad(x64.detach(), (pl, pr)), w64.detach(), None, dilation=d)
    return (y.detach().permute(0, 2, 1), x64.grad.permute(0, 2, 1), w64.grad, b64.grad, ypre.permute(0, 2, 1))


def run_conv_case(cin, cout, k, d, causal, which, act=ACT_NONE, seed=1, cout_true=None):
    """one layer at one length through the real entry points; returns {quantity: error} after asserting family and bounds.
    cout_true: the layer's own channel count where the step pads the weight with zero rows (the 30-channel output layer)."""
    from viai_amd import _lib, ops
    L = lib()
    T, want = length_and_routes(cin, cout, k, d, causal, which)
    desc = TOOL.wavenet_desc(N_STEP, T, cin, cout, k, d, causal)
    dd = ops.conv_desc(*desc)
    assert (dd["OH"], dd["OW"]) == (1, T)
    pl = desc[11]
    pr = desc[16] if desc[16] >= 0 else desc[11]
    ct = cout if cout_true is None else cout_true
    g = _gen(1000 * seed + 7 * cin + cout + d + T)
    x = _uni(g, (N_STEP, T, cin))
    w = torch.randn((cout, cin, k), generator=g) / math.sqrt(cin * k)
    b = _uni(g, (cout,), -0.1, 0.1)
    gy = _uni(g, (N_STEP, T, cout), -1e-3, 1e-3)
    if ct < cout:
        w[ct:], b[ct:], gy[..., ct:] = 0.0, 0.0, 0.0          # WaveNet.forward_nhwc: zero rows; the loss leaves zeros in the padded columns
    y64, dx64, dw64, db64, ypre64 = _conv_truth(x, w[:ct], b[:ct], gy[..., :ct], k, d, pl, pr, act)
    fam = C.create_string_buffer(64)

    def tag():
        n = L.viai_conv2d_last_kernel(fam, 64)
        return n, fam.value.decode()

    xd, wd, bd, gyd = _cuda(x), _cuda(w.unsqueeze(2)), _cuda(b), _cuda(gy)
    s = st()
    errs = {}
    # ---- forward, as ops._conv_fwd calls it
    wp = torch.empty(dd["packed"], device="cuda")
    _lib.check(L.viai_conv2d_pack_fwd(dd["ref"], wd.data_ptr(), wp.data_ptr(), s), "pack_fwd")
    f16 = _fwd_form(desc) == FORM_AMAX
    xa = xd.abs().max().reshape(1).contiguous() if f16 else None

    def fwd(xin, bias, a, amax):
        y = _nan((N_STEP, 1, T, cout))
        _lib.check(L.viai_conv2d_fwd_amax(dd["ref"], xin.data_ptr(), 0, wp.data_ptr(), ptr(bias), y.data_ptr(), 0, a, ptr(amax), s), "viai_conv2d_fwd_amax")
        assert tag() == want[0], ("forward", desc, tag(), want[0])
        return y.reshape(N_STEP, T, cout)
    y = fwd(xd, bd, act, xa)
    errs["y"] = _relerr(y[..., :ct], y64)
    if ct < cout:
        assert bool((y[..., ct:] == 0).all())
    # ---- data gradient: the fp32-form image, no abs-max (ops._conv_grads without a BatchNorm in front)
    # (behind a ReLU the step takes the activation's gradient first, viai_act_bwd_from_output; here with the mask of the fp64 output, so that
    # an output within rounding of the kink cannot put a whole gradient element into the comparison)
    dyd = gyd if act == ACT_NONE else _cuda(gy * (F.pad(y64, (0, cout - ct)) > 0))
    wpd = torch.empty(dd["packed"], device="cuda")
    _lib.check(L.viai_conv2d_pack_dgrad(dd["ref"], wd.data_ptr(), wpd.data_ptr(), s), "pack_dgrad")
    dx = _nan((N_STEP, T, cin))
    _lib.check(L.viai_conv2d_dgrad(dd["ref"], dyd.data_ptr(), wpd.data_ptr(), dx.data_ptr(), 0, s), "viai_conv2d_dgrad")
    assert tag() == want[1], ("data gradient", desc, tag(), want[1])
    errs["dx"] = _relerr(dx, dx64)
    # ---- weight and bias gradient, overwriting and accumulating into non-zero targets
    ws = torch.empty(max(1, dd["ws_floats"]), device="cuda")
    g2 = _gen(5)
    for acc in (0, 1):
        dw0 = (_uni(g2, (cout, cin, 1, k)) * float(dw64.abs().max())).cuda()
        db0 = (_uni(g2, (cout,)) * float(db64.abs().max())).cuda()
        dw = dw0.clone() if acc else _nan((cout, cin, 1, k))
        db = db0.clone() if acc else _nan((cout,))
        _lib.check(L.viai_conv2d_wgrad(dd["ref"], xd.data_ptr(), 0, dyd.data_ptr(), ws.data_ptr(), dw.data_ptr(), db.data_ptr(), acc, s), "viai_conv2d_wgrad")
        assert tag() == want[2], ("weight gradient", desc, tag(), want[2])
        dwk = dw.double().cpu().reshape(cout, cin, k) - (dw0.double().cpu().reshape(cout, cin, k) if acc else 0)
        dbk = db.double().cpu() - (db0.double().cpu() if acc else 0)
        errs["dw.acc%d" % acc] = _relerr(dwk[:ct], dw64)
        errs["db.acc%d" % acc] = _relerr(dbk[:ct], db64)
        if not acc:
            for t in range(k):                                   # a tap whose every read lies in the padding: no product at all
                if k > 1 and causal and (k - 1 - t) * d >= T:
                    assert bool((dw64[:, :, t] == 0).all()) and bool((dwk[:, :, t] == 0).all()), "tap %d lies wholly in the padding" % t
    # ---- adjointness of the linear part: <conv(x), gy> = <x, dgrad(gy)>  (test_step_launches_gpu.py)
    y0 = fwd(xd, None, ACT_NONE, xa)
    dx0 = dx
    if act != ACT_NONE:
        dx0 = _nan((N_STEP, T, cin))
        _lib.check(L.viai_conv2d_dgrad(dd["ref"], gyd.data_ptr(), wpd.data_ptr(), dx0.data_ptr(), 0, s), "viai_conv2d_dgrad")
    lhs = (y0.double() * gyd.double()).sum().item()
    rhs = (xd.double() * dx0.double()).sum().item()
    errs["adj"] = abs(lhs - rhs) / (y0.double().norm() * gyd.double().norm()).item()
    errs["y0"] = _relerr(y0[..., :ct], ypre64)
    # ---- causality: another input from t0 on (same abs-max bound) leaves every earlier output bit for bit (non-causal: every output before t0 - pr)
    t0 = T // 2 + 3 if causal else T - 6
    x2 = x.clone()
    x2[:, t0:] = _uni(g, (N_STEP, T - t0, cin))
    x2d = _cuda(x2)
    both = torch.maximum(xd.abs().max(), x2d.abs().max()).reshape(1).contiguous() if f16 else None
    ya, yb = fwd(xd, bd, act, both), fwd(x2d, bd, act, both)
    keep = t0 - pr
    assert keep > 0 and not torch.equal(ya[:, t0:], yb[:, t0:])
    assert_bitwise(yb[:, :keep], ya[:, :keep], "outputs before t0 = %d (right padding %d)" % (t0, pr))
    torch.cuda.synchronize()
    print("%4d->%-4d k%d d%-3d %-9s T %-5d %-22s %-22s %-22s ks %-3d %s" % (
        cin, ct, k, d, "causal" if causal else "symmetric", T, want[0][1], want[1][1], want[2][1], wgrad_ksplit(desc),
        " ".join("%s %.2e" % kv for kv in sorted(errs.items()))))
    bounds = {"y": TOL["y"], "y0": TOL["y"], "dx": TOL["dx"], "dw.acc0": TOL["dw"], "dw.acc1": TOL["dw"], "db.acc0": TOL["db"], "db.acc1": TOL["db"]}
    bounds["adj"] = adj_bound(N_STEP * T * cout)
    over = {q: (v, bounds[q]) for q, v in errs.items() if not v <= bounds[q]}
    assert not over, (desc, want, over)
    return errs


WHICH = ("train", "ragged", "sk")
# (name, Cin, Cout, k, dilations, act of the forward, Cout of the layer itself where the step pads it)
CONV_LAYERS = [
    ("full.conv", 512, 512, 3, (32,), ACT_NONE, None),          # one dilation at this width: 77 GFLOP of fp64 per length on the CPU
    ("full.cond", 80, 512, 1, (1,), ACT_NONE, None),
    ("full.out", 256, 512, 1, (1,), ACT_NONE, None),
    ("full.skip", 256, 256, 1, (1,), ACT_NONE, None),
    ("full.head1", 256, 256, 1, (1,), ACT_RELU, None),
    ("full.head2", 256, 32, 1, (1,), ACT_NONE, 30),
    ("small.conv", 64, 64, 3, (1, 2, 32, 64), ACT_NONE, None),   # the dilation sweep; at T = 40, d = 32 leaves tap 0 wholly in the padding, d = 64 taps 0 and 1
    ("small.cond", 80, 64, 1, (1,), ACT_NONE, None),
    ("small.out", 32, 64, 1, (1,), ACT_NONE, None),
    ("small.skip", 32, 32, 1, (1,), ACT_NONE, None),
    ("small.head1", 32, 32, 1, (1,), ACT_RELU, None),
    ("small.head2", 32, 32, 1, (1,), ACT_NONE, 30),
    ("deep.conv", 32, 32, 3, (1, 2, 32, 64), ACT_NONE, None),
    ("deep.cond", 80, 32, 1, (1,), ACT_NONE, None),
    ("deep.out", 16, 32, 1, (1,), ACT_NONE, None),
]
CONV_CASES = [(name, cin, cout, k, d, True, which, act, ct) for name, cin, cout, k, ds, act, ct in CONV_LAYERS for d in ds for which in WHICH]
# causal = False: the symmetric padding (k - 1) / 2 * d of ResidualConv1dGLU(causal=False)
CONV_CASES += [("small.conv.symmetric", 64, 64, 3, 2, False, which, ACT_NONE, None) for which in WHICH]
CONV_CASES += [("full.conv.symmetric", 512, 512, 3, 2, False, "sk", ACT_NONE, None)]


@pytest.mark.parametrize("name,cin,cout,k,d,causal,which,act,ct", CONV_CASES, ids=["%s-d%d-%s" % (c[0], c[4], c[6]) for c in CONV_CASES])
def test_conv1d_launch(name, cin, cout, k, d, causal, which, act, ct):
    run_conv_case(cin, cout, k, d, causal, which, act, cout_true=ct)


def test_conv_cases_cover_both_sides_of_every_switch():
    """host only: over CONV_CASES, each pass runs a split-K and a plain kernel -- by family for forward and data gradient, by the split count
    for the weight gradient (its families split inside) -- and the fp32 weight-gradient kernels of the narrow layers are reached"""
    fams = [set(), set(), set()]
    ks = set()
    for name, cin, cout, k, d, causal, which, act, ct in CONV_CASES:
        T, want = length_and_routes(cin, cout, k, d, causal, which)
        for p in range(3):
            assert want[p][0] == 1 and want[p][1], (name, which, p, want)
            fams[p].add(want[p][1])
        ks.add(wgrad_ksplit(TOOL.wavenet_desc(N_STEP, T, cin, cout, k, d, causal)))
    print("forward", sorted(fams[0]), "\ndata gradient", sorted(fams[1]), "\nweight gradient", sorted(fams[2]), "split counts", sorted(ks))
    for p in (0, 1):
        assert any(f.startswith("igemm_sk") for f in fams[p]) and any(f.startswith("igemm") and not f.startswith("igemm_sk") for f in fams[p]), fams[p]
    assert 1 in ks and max(ks) > 1, ks
    assert {"igemm128x256_f16x2", "igemm64x64_f16x2", "igemm128x32_f16x2", "igemm_sk32x32_f16x2"} <= fams[0]
    assert {"igemm128x128_bf16x3", "igemm64x64_bf16x3", "igemm128x32_bf16x3", "igemm_sk32x32_bf16x3"} <= fams[1]
    assert {"wgrad_bf3_bf16x3", "wgrad_mfma_f32", "wgrad32_all_taps_f32"} <= fams[2]


def test_unpadded_output_layer_has_no_backward():
    """Cout = 30: a forward route, but neither gradient -- both entry points refuse on the host, before any launch (the step pads to 32 rows)"""
    from viai_amd import ops
    L = lib()
    for cin in (256, 32):
        desc = TOOL.wavenet_desc(N_STEP, 64, cin, 30, 1)
        r = step_routes(desc)
        assert r[0] == (1, "igemm128x32_f16x2") and r[1] == (0, "") and r[2] == (0, ""), r
        dd = ops.conv_desc(*desc)
        t = torch.zeros(max(dd["packed"], N_STEP * 64 * cin), device="cuda")
        assert L.viai_conv2d_dgrad(dd["ref"], t.data_ptr(), t.data_ptr(), t.data_ptr(), 0, st()) == INVALID
        assert L.viai_conv2d_wgrad(dd["ref"], t.data_ptr(), 0, t.data_ptr(), t.data_ptr(), t.data_ptr(), 0, 0, st()) == INVALID
        assert step_routes(TOOL.wavenet_desc(N_STEP, 64, cin, 32, 1))[1][0] == 1


# ============================================================================================================== B. the other kernels
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("rows,Lc", [(64, 1), (30, 256), (128, 192), (64, 576), (5, 1537)])
def test_weight_norm(rows, Lc, accumulate):
    L = lib()
    g = _gen(11 + rows + Lc)
    v, gg, dw = _uni(g, (rows, Lc)), _uni(g, (rows,), 0.5, 1.5), _uni(g, (rows, Lc))
    dv0, dg0 = _uni(g, (rows, Lc)), _uni(g, (rows,))
    outs = []
    for dt in (torch.float64, torch.float32):
        vv, gv = v.to(dt).requires_grad_(True), gg.to(dt).reshape(rows, 1).requires_grad_(True)
        w = torch._weight_norm(vv, gv, 0)
        w.backward(dw.to(dt))
        dv, dg = vv.grad, gv.grad.reshape(rows)
        if accumulate:
            dv, dg = dv0.to(dt) + dv, dg0.to(dt) + dg
        outs.append((w.detach(), vv.detach().norm(dim=1), dv, dg))
    (w64, n64, dv64, dg64), (w32, n32, dv32, dg32) = outs
    vd, gd, dwd = _cuda(v), _cuda(gg), _cuda(dw)
    wk, nk = _nan((rows, Lc)), _nan((rows,))
    ok(L.viai_weight_norm_fwd(vd.data_ptr(), gd.data_ptr(), wk.data_ptr(), nk.data_ptr(), rows, Lc, st()), "viai_weight_norm_fwd")
    what = "weight_norm %dx%d acc%d " % (rows, Lc, accumulate)
    check(wk, w64, w32, what + "w", "abs")
    check(nk, n64, n32, what + "norm", "fro")
    dvk, dgk = (_cuda(dv0), _cuda(dg0)) if accumulate else (_nan((rows, Lc)), _nan((rows,)))
    ok(L.viai_weight_norm_bwd(dwd.data_ptr(), vd.data_ptr(), gd.data_ptr(), nk.data_ptr(), dvk.data_ptr(), dgk.data_ptr(), rows, Lc, accumulate, st()),
       "viai_weight_norm_bwd")
    if Lc == 1:
        # dv = g / n (dw - v <dw, v> / n^2) is exactly 0: what is left is rounding of v <dw, v> / n^2 against dw -- one rounding each for dw v, v v, the
        # square root (counted twice), n n, the quotient and the product: at most 7 x 2^-24 = 3.5 ulp of |g / n dw|; accumulating adds one rounding of the sum
        lead = (gg.detach().double() / v.detach().double().abs().reshape(rows) * dw.double().abs().reshape(rows)).reshape(rows, 1)
        base = dv0.double() if accumulate else torch.zeros(rows, 1, dtype=torch.float64)
        resid = (host(dvk).double() - base).abs()
        tol = 4.0 * EPS32 * lead + (EPS32 * base.abs() if accumulate else 0.0)
        print("%-58s worst |dv - base| / (ulp of |g/n dw|) %.2f" % (what + "dv", float((resid / (EPS32 * lead)).max())))
        assert bool((resid <= tol).all()), (what, float((resid / tol).max()))
    else:
        check(dvk, dv64, dv32, what + "dv", "abs")
    check(dgk, dg64, dg32, what + "dg", "fro")


def _glu_truth(y, yc, dz, dt):
    H = y.shape[1] // 2
    yy = y.to(dt).requires_grad_(True)
    cc = yc.to(dt).requires_grad_(True) if yc is not None else None
    s = yy if cc is None else yy + cc
    z = torch.tanh(s[:, :H]) * torch.sigmoid(s[:, H:])
    z.backward(dz.to(dt))
    return z.detach(), yy.grad, (cc.grad if cc is not None else None)


def _glu_case(rows, H, with_yc, g):
    L = lib()
    y, dz = _uni(g, (rows, 2 * H), -8.0, 8.0), _uni(g, (rows, H))
    yc = _uni(g, (rows, 2 * H), -8.0, 8.0) if with_yc else None
    z64, dy64, dc64 = _glu_truth(y, yc, dz, torch.float64)
    z32, dy32, dc32 = _glu_truth(y, yc, dz, torch.float32)
    pre = y.double() + (yc.double() if with_yc else 0.0)
    sat = float((pre.abs() > 5.0).double().mean())                 # tanh within 1e-4 of +-1, the sigmoid within 7e-3 of 0 or 1
    assert rows * H < 1000 or 0.1 < sat < 0.9, sat                 # part of the tensor saturates, part does not
    yd, dzd, ycd = _cuda(y), _cuda(dz), (_cuda(yc) if with_yc else None)
    zk, dyk = _nan((rows, H)), _nan((rows, 2 * H))
    ok(L.viai_glu_fwd(yd.data_ptr(), ptr(ycd), zk.data_ptr(), rows, H, st()), "viai_glu_fwd")
    ok(L.viai_glu_bwd(dzd.data_ptr(), yd.data_ptr(), ptr(ycd), dyk.data_ptr(), rows, H, st()), "viai_glu_bwd")
    what = "glu %dx%d yc %d " % (rows, H, with_yc)
    check(zk, z64, z32, what + "z", "abs")
    check(dyk, dy64, dy32, what + "dy", "abs")
    if with_yc:
        check(dyk, dc64, dc32, what + "dyc (the same tensor)", "abs")


@pytest.mark.parametrize("with_yc", [False, True], ids=["yc_null", "yc_set"])
@pytest.mark.parametrize("rows,H", [(3, 4), (130, 32), (77, 256)])
def test_glu(rows, H, with_yc):
    _glu_case(rows, H, with_yc, _gen(21 + rows))


def test_glu_grid_cap():
    rows, H = 8200, 1024
    assert rows * (H // 4) > 8192 * 256
    _glu_case(rows, H, False, _gen(23))
    assert lib().viai_glu_fwd(0, 0, 0, 4, 6, st()) == INVALID          # H % 4


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("rows", [1, 1000, 3073])
@pytest.mark.parametrize("Cc", [64, 96, 2048])
def test_outer(Cc, rows, accumulate):
    L = lib()
    nb = L.viai_outer_bwd_blocks(rows)
    rpb = -(-rows // nb)
    if rows == 3073:                                               # several partial blocks, the last one short (766 of 769 rows), no row count a multiple of 256 / cgw
        assert nb == 4 and rows - (nb - 1) * rpb not in (0, rpb)
    else:
        assert nb == 1
    g = _gen(31 + Cc + rows)
    x, w, b, dy = _uni(g, (rows,)), _uni(g, (Cc,)), _uni(g, (Cc,)), _uni(g, (rows, Cc))
    dw0, db0 = _uni(g, (Cc,), -30.0, 30.0), _uni(g, (Cc,), -30.0, 30.0)
    outs = []
    for dt in (torch.float64, torch.float32):
        xx, ww, bb, gy = x.to(dt), w.to(dt), b.to(dt), dy.to(dt)
        dw, db = (gy * xx[:, None]).sum(0), gy.sum(0)
        if accumulate:
            dw, db = dw0.to(dt) + dw, db0.to(dt) + db
        outs.append((xx[:, None] * ww + bb, dw, db))
    (y64, dw64, db64), (y32, dw32, db32) = outs
    xd, wd, bd, dyd = _cuda(x), _cuda(w), _cuda(b), _cuda(dy)
    yk = _nan((rows, Cc))
    ok(L.viai_outer_fwd(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), yk.data_ptr(), rows, Cc, st()), "viai_outer_fwd")
    what = "outer C%d rows %d acc%d " % (Cc, rows, accumulate)
    check(yk, y64, y32, what + "y", "abs")
    part = _nan((2 * Cc * nb,))
    dwk, dbk = (_cuda(dw0), _cuda(db0)) if accumulate else (_nan((Cc,)), _nan((Cc,)))
    ok(L.viai_outer_bwd(dyd.data_ptr(), xd.data_ptr(), part.data_ptr(), dwk.data_ptr(), dbk.data_ptr(), rows, Cc, accumulate, st()), "viai_outer_bwd")
    check(dwk, dw64, dw32, what + "dw", "fro")
    check(dbk, db64, db32, what + "db", "fro")
    assert L.viai_outer_fwd(0, 0, 0, 0, rows, 6, st()) == INVALID and L.viai_outer_bwd(0, 0, 0, 0, 0, rows, 6, 0, st()) == INVALID      # C % 4


def _up_truth(x, w, b, dy, KH, S, dt):
    xx, ww, bb = x.to(dt).requires_grad_(True), w.to(dt).requires_grad_(True), b.to(dt).requires_grad_(True)
    pre = F.conv_transpose2d(xx.unsqueeze(1), ww, bb, stride=(1, S), padding=((KH - 1) // 2, 0)).squeeze(1)
    y = torch.relu(pre)
    y.backward(dy.to(dt))
    return pre.detach(), y.detach(), xx.grad, ww.grad, bb.grad


# KH: the two instances of the host dispatch (viai_upsample_fwd / _bwd: KH == 3 or 1, anything else refused)
@pytest.mark.parametrize("B,Fq,T", [(1, 1, 3), (2, 80, 7), (1, 5, 300)])
@pytest.mark.parametrize("S", [4, 5, 16])
@pytest.mark.parametrize("KH", [1, 3])
def test_upsample(KH, S, B, Fq, T):
    L = lib()
    g = _gen(59 + 100 * KH + S + T)
    x, w, b = _uni(g, (B, Fq, T)), _uni(g, (1, 1, KH, S)), _uni(g, (1,), -0.2, 0.2)
    dy = _uni(g, (B, Fq, T * S))
    for _ in range(50):                                            # no pre-activation within 1e-5 of the kink: the fp32 mask is then the fp64 one
        pre64 = _up_truth(x, w, b, dy, KH, S, torch.float64)[0]
        if float(pre64.abs().min()) > 1e-5:
            break
        b = b + 7e-4
    assert float(pre64.abs().min()) > 1e-5
    neg = float((pre64 < 0).double().mean())
    assert 0.2 <= neg <= 0.8, neg                                  # the ReLU mask matters in the backward
    _, y64, dx64, dw64, db64 = _up_truth(x, w, b, dy, KH, S, torch.float64)
    _, y32, dx32, dw32, db32 = _up_truth(x, w, b, dy, KH, S, torch.float32)
    xd, wd, bd, dyd = _cuda(x), _cuda(w), _cuda(b), _cuda(dy)
    yk = _nan((B, Fq, T * S))
    ok(L.viai_upsample_fwd(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), yk.data_ptr(), B, Fq, T, KH, S, st()), "viai_upsample_fwd")
    what = "upsample KH%d S%d %dx%dx%d " % (KH, S, B, Fq, T)
    check(yk, y64, y32, what + "y", "abs")
    assert torch.equal(host(yk) > 0, y64 > 0)
    part = _nan(((KH * 16 + 1) * L.viai_upsample_bwd_blocks(),))
    dw0, db0 = _uni(g, (1, 1, KH, S), -3.0, 3.0), _uni(g, (1,), -3.0, 3.0)
    for with_dx in (False, True):
        for acc in (0, 1):
            dxk = _nan((B, Fq, T)) if with_dx else None
            dwk, dbk = (_cuda(dw0), _cuda(db0)) if acc else (_nan((1, 1, KH, S)), _nan((1,)))
            ok(L.viai_upsample_bwd(dyd.data_ptr(), yk.data_ptr(), xd.data_ptr(), wd.data_ptr(), part.data_ptr(), ptr(dxk), dwk.data_ptr(), dbk.data_ptr(),
                                   B, Fq, T, KH, S, acc, st()), "viai_upsample_bwd")
            tag = what + "dx %d acc%d " % (with_dx, acc)
            if with_dx:
                check(dxk, dx64, dx32, tag + "dx", "abs")
            # KH 1, S 16 on the 1 x 1 x 3 map: db sums 48 masked gradients, and torch's fp32 sum (also behind db0) happens to be the rounded truth
            # itself, error 0, while the kernel's 512 block partials added in another order land 1.3 / 1.8 ulp off.  No fp32 sum in another order can
            # be held to 0: this one case gets 2 ulp of the output instead of 4 x 0; every other case keeps the plain rule
            fl = 2.0 if (KH, S, B, Fq, T) == (1, 16, 1, 1, 3) else 0.0
            if acc:
                check(dwk, dw0.double() + dw64, dw0 + dw32, tag + "dw", "fro")
                check(dbk, db0.double() + db64, db0 + db32, tag + "db", "fro", floor_ulps=fl)
            else:
                check(dwk, dw64, dw32, tag + "dw", "fro")
                check(dbk, db64, db32, tag + "db", "fro", floor_ulps=fl)


def test_upsample_refuses_other_windows():
    L = lib()
    t = torch.zeros(4096, device="cuda")
    p = t.data_ptr()
    assert L.viai_upsample_fwd(p, p, p, p, 1, 1, 3, 2, 4, st()) == INVALID
    assert L.viai_upsample_bwd(p, p, p, p, p, p, p, p, 1, 1, 3, 2, 4, 0, st()) == INVALID
    assert L.viai_upsample_bwd(p, p, p, p, p, p, p, p, 1, 1, 3, 3, 17, 0, st()) == INVALID


def _mol_truth(yh, y, mask, dt):
    """oracle/wavenet_oracle.py on rows: yh (rows, 30), y (rows,), mask (rows,) or None -> (loss rows, loss, d loss / d yh, row weights)"""
    from oracle import wavenet_oracle as W
    a = yh.to(dt).requires_grad_(True)
    rows = W.mol_loss_rows(a.t().unsqueeze(0), y.to(dt).reshape(1, -1, 1), 65536, math.log(1e-14)).reshape(-1)
    m = torch.ones_like(rows) if mask is None else mask.to(dt)
    loss = (rows * m).sum() / m.sum()
    loss.backward()
    return rows.detach(), loss.detach().reshape(1), a.grad, m / m.sum()


@pytest.mark.parametrize("rows,pitch,mask_kind,want_grad", [(300, 32, "null", True), (300, 40, "zero_rows", True), (1000, 32, "ones", False),
                                                            (77, 40, "null", False), (1000, 40, "zero_rows", True)])
def test_mol_loss(rows, pitch, mask_kind, want_grad):
    L = lib()
    g = _gen(51 + rows + pitch)
    yh = _uni(g, (rows, 30), -2.0, 2.0)
    yh[:8, 20:30] = 6.0                                            # huge scales: the cdf_delta <= 1e-5 branch
    yh[8:12, 20:30] = -40.0                                        # below log_scale_min: clamped, zero gradient
    y = _uni(g, (rows,), -0.99, 0.99)
    y[0], y[20], y[30], y[rows - 1] = -1.0, 1.0, 0.9995, -0.9995
    mask = None
    if mask_kind == "ones":
        mask = torch.ones(rows)
    elif mask_kind == "zero_rows":
        mask = torch.ones(rows)
        mask[5:9], mask[rows - 40:] = 0.0, 0.0
    r64, l64, d64, w64 = _mol_truth(yh, y, mask, torch.float64)
    r32, l32, d32, w32 = _mol_truth(yh, y, mask, torch.float32)
    rowsd = torch.full((rows, pitch), 1e30)                        # the columns past 3 K are never read
    rowsd[:, :30] = yh
    yhd, yd, md = _cuda(rowsd), _cuda(y), (_cuda(mask) if mask is not None else None)
    lr, wr, lo = _nan((rows,)), _nan((rows,)), _nan((1,))
    dyh = _nan((rows, pitch)) if want_grad else None
    ok(L.viai_mol_loss(yhd.data_ptr(), yd.data_ptr(), ptr(md), lr.data_ptr(), wr.data_ptr(), lo.data_ptr(), ptr(dyh), rows, pitch, 10, 65536.0,
                       math.log(1e-14), st()), "viai_mol_loss")
    what = "mol_loss rows %d pitch %d mask %s " % (rows, pitch, mask_kind)
    check(lr, r64, r32, what + "loss rows", "abs")
    check(lo, l64, l32, what + "loss", "fro")
    check(wr, w64, w32, what + "row weights", "abs")
    if want_grad:
        assert bool((host(dyh)[:, 30:] == 0).all()), "columns >= 30 of dyhat"
        check(dyh[:, :30], d64, d32, what + "dyhat", "abs")
        if mask is not None:
            assert bool((host(dyh)[mask == 0] == 0).all()), "rows of weight zero"
    assert L.viai_mol_loss(yhd.data_ptr(), yd.data_ptr(), 0, lr.data_ptr(), wr.data_ptr(), lo.data_ptr(), 0, rows, 28, 10, 65536.0, -32.0, st()) == INVALID
    assert L.viai_mol_loss(yhd.data_ptr(), yd.data_ptr(), 0, lr.data_ptr(), wr.data_ptr(), lo.data_ptr(), 0, rows, pitch, 5, 65536.0, -32.0, st()) == INVALID


@pytest.mark.parametrize("n4", [1, 8192 * 256 + 777])
def test_elementwise_bitwise(n4):
    """relu, a * s (viai_add_scale with b = NULL) and the in-place d *= *g: one select or one multiply per element"""
    L = lib()
    n = 4 * n4
    g = _gen(61)
    a = _uni(g, (n,), -2.0, 2.0)
    a[0], a[1], a[n - 1] = 0.0, -0.0, -1.5
    ad = _cuda(a)
    out = _nan((n,))
    ok(L.viai_relu_fwd(ad.data_ptr(), out.data_ptr(), n, st()), "viai_relu_fwd")
    assert_bitwise(out, torch.where(a > 0, a, torch.zeros(())), "relu_fwd n = %d" % n)
    s = torch.tensor(math.sqrt(0.5), dtype=torch.float32)
    out = _nan((n,))
    ok(L.viai_add_scale(ad.data_ptr(), 0, out.data_ptr(), float(s), n, st()), "viai_add_scale")
    assert_bitwise(out, a * s, "add_scale b = NULL n = %d" % n)
    # scale_by_scalar counts elements, not float4s: n4 + 3 elements of the same draw (past the cap: 8192 * 256 + 780)
    m = n4 + 3
    gs = torch.tensor([-0.37], dtype=torch.float32)
    d = ad[:m].clone()
    ok(L.viai_scale_by_scalar(d.data_ptr(), _cuda(gs).data_ptr(), m, st()), "viai_scale_by_scalar")
    assert_bitwise(d, a[:m] * gs, "scale_by_scalar n = %d" % m)
    assert L.viai_relu_fwd(ad.data_ptr(), out.data_ptr(), 6, st()) == INVALID and L.viai_add_scale(ad.data_ptr(), 0, out.data_ptr(), 1.0, 6, st()) == INVALID
