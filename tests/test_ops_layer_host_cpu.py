"""The host path of the fused layer (viai_amd/ops.py, viai_amd/torch_ops.py), pinned without a GPU.  Nothing is launched.

  * `ops._layer_spec` -- the one builder of a layer's configuration -- over its whole input space against the expressions it replaced (the `cfg` dicts
    of `conv_bn_act`, `conv_bn_act_cout1` and `torch_ops._cfg`), written out below as they stood.
  * `ops._layer_desc` -- the key it hands to `conv_desc`, the channel-stride-4 rule of the frame tensors included.
  * the launch sequences: `_lib.load` hands out a recording stand-in that forwards the host queries to the real library (it loads without a device)
    and logs every other entry point; the layers run forward and backward on CPU tensors (nothing is computed) and the log of every case must be the
    one recorded from the code as it stood before the spec: call names, scalar arguments, descriptors, and which pointers were null.
"""
import ctypes as C
import gc
import itertools
import weakref

import pytest
import torch

BOOLS = (False, True)
ACT_NONE, ACT_RELU, ACT_LRELU, ACT_SIGMOID = 0, 1, 2, 3
QUERIES = ("viai_conv2d_out_hw", "viai_conv2d_stat_geom", "viai_conv2d_stat_tiles", "viai_conv2d_packed_floats", "viai_conv2d_wgrad_ws_bytes",
           "viai_class_embed_bwd_segments", "viai_abi_version")


class Recorder:
    """stands in for the loaded library: host queries go to the real one, every other entry point appends (name, arguments) to `log` and returns 0.
    Arguments: scalars as they are, a descriptor as the tuple of its fields, pointers numbered by first appearance (0 stays 0)."""

    def __init__(self, real, signatures):
        self.real, self.sig, self.log, self.ptrs = real, signatures, [], {}

    def _arg(self, a, ctype):
        if ctype is C.c_void_p:
            return 0 if not a else "p%d" % self.ptrs.setdefault(int(a), len(self.ptrs) + 1)
        if hasattr(a, "_obj"):                                           # C.byref(Conv2dDesc)
            return tuple(getattr(a._obj, f) for f, _ in a._obj._fields_)
        return a

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if name in QUERIES or name.endswith("_ok") or name.endswith("_blocks"):
            return fn
        types = self.sig[name][1]

        def launch(*args):
            assert len(args) == len(types), name
            self.log.append((name, tuple(self._arg(a, t) for a, t in zip(args, types))))
            return 0
        return launch


def scalars(log, nullness=True):
    """a log without the pointer numbering: "p" for a pointer and 0 for a null one, or (nullness=False) no pointer arguments at all"""
    from viai_amd._lib import SIGNATURES
    out = []
    for name, args in log:
        keep = [("p" if isinstance(a, str) else a) for a, t in zip(args, SIGNATURES[name][1]) if nullness or t is not C.c_void_p]
        out.append((name, tuple(keep)))
    return out


def _require_without_device(*tensors):
    """ops._require minus its device check"""
    for t in tensors:
        if t is None:
            continue
        if getattr(t, "_viai_p16", False):
            raise TypeError("this op does not take a pre-split (P16) tensor; ops.p16_decode() gives its fp32 values")
        if t.dtype != torch.float32:
            raise TypeError("viai ops are fp32, got %s" % t.dtype)


def make_harness(monkeypatch):
    """the fused layer without a device: returns a function that installs a fresh Recorder (and forgets the module's pooled buffers, so that every
    case starts from the same state)"""
    from viai_amd import _lib, ops
    real = _lib.load()
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    monkeypatch.setattr(ops, "_require", _require_without_device)
    monkeypatch.setattr(ops, "DIRECT_GRAD", False)
    monkeypatch.setattr(ops, "WGRAD_STREAM", None)
    monkeypatch.setattr(ops, "P16", True)
    monkeypatch.setattr(ops, "F16_BACKWARD", True)
    monkeypatch.setattr(ops, "_amax_managed", False)
    monkeypatch.delenv("VIAI_WGRAD_PATCH_S2", raising=False)
    monkeypatch.delenv("VIAI_CIN1_BN_DGRAD", raising=False)

    def install():
        for pool in (ops._scratch_pool, ops._free_ring, ops._unit_amax):
            pool.clear()
        rec = Recorder(real, _lib.SIGNATURES)
        monkeypatch.setattr(_lib, "load", lambda: rec)
        return rec
    return install


@pytest.fixture
def harness(monkeypatch):
    return make_harness(monkeypatch)


# ------------------------------------------------------------------------------------------- _layer_spec against the expressions it replaced
def old_cfg(ops, x, x2, weight, bias, bn, kernel, stride, padding, transposed, act, training, dilation, padding2, xmask, pool, upsample, out_p16):
    """ops.conv_bn_act before the spec: the dict it built (xmask already decided) and the statistics tensors it passed to apply"""
    cfg = {"k": tuple(kernel), "s": tuple(stride), "p": tuple(padding), "transposed": bool(transposed),
           "act": int(act), "training": bool(training), "momentum": 0.1, "eps": ops.BN_EPS,
           "d": tuple(dilation), "p2": tuple(padding2), "xa_in": (ops.amax_of(x), ops.amax_of(x2)), "xmask": xmask,
           "pool": tuple(int(v) for v in pool) if pool is not None else None,
           "up": (int(upsample[0]), int(upsample[1])) if upsample is not None else None,
           "p16_out": bool(out_p16) and bn is not None and isinstance(bn, torch.nn.modules.batchnorm._BatchNorm) and bn.weight is not None}
    if bn is not None:
        cfg["momentum"] = 0.1 if bn.momentum is None else float(bn.momentum)
        cfg["eps"] = float(bn.eps)
        track = bn.track_running_stats and bn.running_mean is not None
        if not training and not track:
            cfg["training"] = True
        if ops.DIRECT_GRAD:
            cfg["gt"] = tuple(p.grad if (p is not None and p.is_leaf and p.requires_grad and p.grad is not None) else None
                              for p in (weight, bias, bn.weight, bn.bias))
        return cfg, (bn.running_mean if track else None, bn.running_var if track else None, bn.num_batches_tracked if (track and cfg["training"]) else None)
    if ops.DIRECT_GRAD:
        cfg["gt"] = tuple(p.grad if (p is not None and p.is_leaf and p.requires_grad and p.grad is not None) else None
                          for p in (weight, bias, None, None))
    return cfg, (None, None, None)


def old_cfg_pair(ops, x, x2, weight, bias, bn, weight2, bias2, kernel, stride, padding, transposed, act, transposed2, act2, training):
    """ops.conv_bn_act_cout1 before the spec"""
    cfg = {"k": tuple(kernel), "s": tuple(stride), "p": tuple(padding), "transposed": bool(transposed), "act": int(act), "training": bool(training),
           "momentum": 0.1 if bn.momentum is None else float(bn.momentum), "eps": float(bn.eps), "transposed2": bool(transposed2),
           "act2": int(act2), "xa_in": (ops.amax_of(x), ops.amax_of(x2))}
    track = bn.track_running_stats and bn.running_mean is not None
    if not training and not track:
        cfg["training"] = True
    if ops.DIRECT_GRAD:
        def tgt(p):
            return p.grad if (p is not None and p.is_leaf and p.requires_grad and p.grad is not None) else None
        cfg["gt"] = tuple(tgt(p) for p in (weight, bias, bn.weight, bn.bias))
        cfg["gt2"] = (tgt(weight2), tgt(bias2))
    return cfg, (bn.running_mean if track else None, bn.running_var if track else None, bn.num_batches_tracked if (track and cfg["training"]) else None)


def old_cfg_torch_ops(kernel, stride, padding, transposed, act, training, momentum, eps, gamma, running_mean, running_var):
    """torch_ops._cfg and the resolution behind it in the registered forward"""
    cfg = {"k": tuple(kernel), "s": tuple(stride), "p": tuple(padding), "transposed": bool(transposed), "act": int(act), "training": bool(training),
           "momentum": float(momentum), "eps": float(eps), "d": (1, 1), "p2": (-1, -1), "xa_in": (None, None), "xmask": None, "pool": None, "up": None,
           "p16_out": False}
    track = running_mean is not None and running_var is not None
    if gamma is not None and not training and not track:
        cfg["training"] = True
    return cfg


SPEC_KEYS = {"k": "k", "s": "s", "p": "p", "transposed": "transposed", "d": "d", "p2": "p2", "act": "act", "training": "training", "momentum": "momentum",
             "eps": "eps", "pool": "pool", "up": "up", "p16_out": "p16_out", "xmask": "xmask", "xa_in": "xa_in", "transposed2": "transposed2", "act2": "act2"}
SPEC_DEFAULTS = {"d": (1, 1), "p2": (-1, -1), "pool": None, "up": None, "p16_out": False, "xmask": None, "transposed2": False, "act2": ACT_NONE}


def same(a, b):
    """equal values, tensors by identity"""
    if isinstance(a, tuple) and isinstance(b, tuple):
        return len(a) == len(b) and all(same(u, v) for u, v in zip(a, b))
    if isinstance(a, torch.Tensor) or isinstance(b, torch.Tensor):
        return a is b
    return type(a) is type(b) and a == b


def check_spec(spec, cfg, n_gt=(4, 2)):
    """every field of the spec against the dict it replaces (a key the dict did not have: the default its readers assumed)"""
    assert set(spec._fields) == set(SPEC_KEYS) | {"gt", "gt2"}
    for f in SPEC_KEYS:
        assert same(getattr(spec, f), cfg.get(f, SPEC_DEFAULTS.get(f))), (f, getattr(spec, f), cfg.get(f))
    assert same(spec.gt, cfg.get("gt") or (None,) * 4) and same(spec.gt2, cfg.get("gt2") or (None,) * 2)
    assert (len(spec.gt), len(spec.gt2)) == n_gt


def _params():
    """(weight, bias) holders: with and without .grad, requires_grad, leafness; no bias"""
    def par(shape, grad, req=True):
        p = torch.nn.Parameter(torch.zeros(shape), requires_grad=req)
        if grad:
            p.grad = torch.zeros(shape)
        return p
    w = (4, 4, 3, 3)
    return [(par(w, True), par(4, True)), (par(w, True), par(4, False)), (par(w, False), None), (par(w, True, req=False), par(4, True)),
            (par(w, True) * 1.0, par(4, True)), (torch.zeros(w), par(4, True) + 0.0)]


def _bns():
    out = {"none": None, "tracking": torch.nn.BatchNorm2d(4), "no running statistics": torch.nn.BatchNorm2d(4, track_running_stats=False),
           "momentum None": torch.nn.BatchNorm2d(4, momentum=None, eps=1e-3), "no affine": torch.nn.BatchNorm2d(4, affine=False)}
    out["tracking"].weight.grad, out["tracking"].bias.grad = torch.zeros(4), torch.zeros(4)
    out["momentum None"].weight.grad = torch.zeros(4)
    return out


def test_layer_spec_agrees_with_the_expressions_it_replaced(monkeypatch):
    from viai_amd import ops
    x, x2 = _tagged(torch.zeros(1, 8, 8, 4)), torch.zeros(1, 8, 8, 4)
    mask = torch.ones(1, 8)
    rows = 0
    for direct, training, (bname, bn), (weight, bias) in itertools.product(BOOLS, BOOLS, _bns().items(), _params()):
        monkeypatch.setattr(ops, "DIRECT_GRAD", direct)
        for pool, up, out_p16, xmask, second in itertools.product((None, [3, 2, 1]), (None, (16.0, 16)), BOOLS, (None, mask), (None, x2)):
            geo = dict(kernel=[3, 3], stride=(2, 1), padding=[1, 1], transposed=second is not None, act=ACT_LRELU)
            cfg, stats = old_cfg(ops, x, second, weight, bias, bn, training=training, dilation=[2, 2], padding2=(0, 1), xmask=xmask, pool=pool, upsample=up,
                                 out_p16=out_p16, **geo)
            spec, got = ops._layer_spec((weight, bias), bn, training=training, dilation=[2, 2], padding2=(0, 1), xmask=xmask, pool=pool, upsample=up,
                                        out_p16=out_p16, xa_in=(ops.amax_of(x), ops.amax_of(second)), **geo)
            check_spec(spec, cfg)
            assert same(got, ((bn.weight, bn.bias) if bn is not None else (None, None)) + stats), (bname, training)
            rows += 1
        if bn is not None:
            w2, b2 = _params()[rows % 2]
            geo = dict(kernel=(3, 3), stride=(1, 1), padding=(1, 1), transposed=False, act=ACT_RELU)
            cfg, stats = old_cfg_pair(ops, x, None, weight, bias, bn, w2, b2, transposed2=True, act2=ACT_SIGMOID, training=training, **geo)
            spec, got = ops._layer_spec((weight, bias), bn, training=training, xa_in=(ops.amax_of(x), None), params2=(w2, b2), transposed2=True, act2=ACT_SIGMOID, **geo)
            check_spec(spec, cfg)
            assert same(got, (bn.weight, bn.bias) + stats)
    assert rows == 2 * 2 * 5 * 6 * 32
    # the registered op: tensors in place of the module, no gradient target whatever the switch says
    monkeypatch.setattr(ops, "DIRECT_GRAD", True)
    weight, bias = _params()[0]
    for training, (gamma, rm, rv) in itertools.product(BOOLS, ((None, None, None), (torch.ones(4), None, None), (torch.ones(4), torch.zeros(4), torch.ones(4)))):
        from types import SimpleNamespace
        geo = dict(kernel=[3, 3], stride=[1, 1], padding=[1, 1], transposed=False, act=ACT_RELU, training=training)
        cfg = old_cfg_torch_ops(momentum=0.3, eps=1e-3, gamma=gamma, running_mean=rm, running_var=rv, **geo)
        bn = None if gamma is None else SimpleNamespace(weight=gamma, bias=None, running_mean=rm, running_var=rv, num_batches_tracked=None,
                                                        track_running_stats=rm is not None, momentum=0.3, eps=1e-3)
        spec, got = ops._layer_spec((weight, bias), bn, direct=False, **geo)
        if gamma is None:
            cfg["momentum"], cfg["eps"] = 0.1, ops.BN_EPS            # (no BatchNorm: nothing reads them)
        check_spec(spec, cfg)
        assert same(got, (gamma, None, rm, rv, None))


# ------------------------------------------------------------------------------------------------------------------------------ _layer_desc
def test_layer_desc_hands_conv_desc_the_key_of_the_layer(monkeypatch):
    from viai_amd import ops
    keys = []
    monkeypatch.setattr(ops, "conv_desc", lambda *key: keys.append(key) or key)
    conv, tconv = torch.zeros(48, 32, 3, 5), torch.zeros(32, 48, 3, 5)                        # nn.Conv2d / nn.ConvTranspose2d layouts of 32 -> 48 channels
    assert ops._layer_desc((2, 8, 6, 32), 0, conv, (3, 5), (2, 1), (1, 2), False) == (2, 8, 6, 32, 0, 48, 3, 5, 2, 1, 1, 2, 0, 1, 1, -1, -1)
    assert ops._layer_desc((2, 8, 6, 32), 0, tconv, (3, 5), (2, 1), (1, 2), True) == (2, 8, 6, 32, 0, 48, 3, 5, 2, 1, 1, 2, 1, 1, 1, -1, -1)
    assert ops._layer_desc((2, 8, 6, 20), 12, conv, (3, 5), (1, 1), (1, 2), False, (2, 3), (0, 1)) == (2, 8, 6, 20, 12, 48, 3, 5, 1, 1, 1, 2, 0, 2, 3, 0, 1)
    assert ops._layer_desc((2, 8, 6, 20), 12, tconv, (3, 5), (1, 1), (1, 2), True, p2=(0, 1)) == (2, 8, 6, 20, 12, 48, 3, 5, 1, 1, 1, 2, 1, 1, 1, 0, 1)
    # frames stored with channel stride 4: a weight of two or three input channels reads the first channels of a four-channel tensor, alone
    for cin_w, transposed, C2 in itertools.product((1, 2, 3, 4), BOOLS, (0, 4)):
        w = torch.zeros(cin_w + C2, 16, 3, 3) if transposed else torch.zeros(16, cin_w + C2, 3, 3)
        C1 = cin_w if (C2 == 0 and cin_w in (2, 3)) else 4
        assert ops._layer_desc((1, 8, 8, 4), C2, w, (3, 3), (1, 1), (1, 1), transposed) == (1, 8, 8, C1, C2, 16, 3, 3, 1, 1, 1, 1, int(transposed), 1, 1, -1, -1)
    assert len(keys) == 4 + 16
    # the spec's geometry, as the forwards pass it
    spec, _ = ops._layer_spec((conv, None), None, kernel=[3, 5], stride=[2, 1], padding=[1, 2], transposed=False, act=0, training=True, dilation=[1, 2], padding2=[2, 2])
    assert ops._layer_desc((2, 8, 6, 32), 0, conv, spec.k, spec.s, spec.p, spec.transposed, spec.d, spec.p2) == (2, 8, 6, 32, 0, 48, 3, 5, 2, 1, 1, 2, 0, 1, 2, 2, 2)


# ------------------------------------------------------------------------------------------------------------------------------ the cases
def _x(*shape):
    return torch.zeros(shape, requires_grad=True)


def _w(cout, cin, kh=3, kw=3, grad=False):
    p = torch.nn.Parameter(torch.zeros(cout, cin, kh, kw))
    if grad:
        p.grad = torch.zeros_like(p)
    return p


def _b(c, grad=False):
    p = torch.nn.Parameter(torch.zeros(c))
    if grad:
        p.grad = torch.zeros_like(p)
    return p


def _bn(c, grad=False, **kw):
    bn = torch.nn.BatchNorm2d(c, **kw)
    if grad:
        bn.weight.grad, bn.bias.grad = torch.zeros(c), torch.zeros(c)
    return bn


def _tagged(t):
    t._viai_amax = torch.ones(1)
    return t


def _with_twin(x):
    """x as a residual join leaves it: fp32, with a pre-split copy beside it"""
    twin = _tagged(torch.zeros(x.shape))
    twin._viai_p16 = True
    _tagged(x)._viai_twin = twin
    return x


def _back(z):
    torch.autograd.backward(z, torch.ones_like(z))


K3 = dict(kernel=(3, 3), padding=(1, 1))
SMALL = (1, 8, 8, 32)                       # no capability bit matters
PLANES = (1, 128, 128, 32)                  # -> 32 channels, 3 x 3: P16_OK_FWD_X | DGRAD_DY | WGRAD_DY | WGRAD_X (the smallest such row of conv_routes.json)
WGRAD_X = (2, 80, 208, 32)                  # -> 128 channels, 3 x 3 stride 2: P16_OK_WGRAD_DY | WGRAD_X only (the smallest such row)


def _layer(ops, shape=SMALL, cout=32, bn=True, **kw):
    kw = {**K3, "act": ACT_RELU, **kw}
    return ops.conv_bn_act(_x(*shape), _w(cout, shape[3]), None, _bn(cout) if bn else None, **kw)


def _res(shape=SMALL, cout=32, stride=1):
    return _tagged(_x(shape[0], shape[1] // stride, shape[2] // stride, cout))


def case_plain(ops):
    return _layer(ops, act=ACT_LRELU)


def case_plain_out_p16(ops):
    return _layer(ops, act=ACT_LRELU, out_p16=True)


def case_up(ops):
    return _layer(ops, upsample=(16, 16))


def case_up_out_p16(ops):
    return _layer(ops, upsample=(16, 16), out_p16=True)


def case_res(ops):
    return _layer(ops, residual=_res())


def case_res_out_p16(ops):
    return _layer(ops, residual=_res(), out_p16=True)


def case_pool(ops):
    return _layer(ops, pool=(3, 2, 1))


def case_pool_out_p16(ops):
    return _layer(ops, pool=(3, 2, 1), out_p16=True)


def case_planes_layer(ops):
    return _layer(ops, PLANES, out_p16=True)


def case_res_twin_consumed(ops):
    x = _with_twin(_x(*PLANES))
    return ops.conv_bn_act(x, _w(32, 32), None, _bn(32), act=ACT_RELU, residual=_res(PLANES), out_p16=True, **K3)


def case_res_twin_for_the_weight_gradient(ops):
    x = _with_twin(_x(*WGRAD_X))
    return ops.conv_bn_act(x, _w(128, 32), None, _bn(128), act=ACT_RELU, residual=_res(WGRAD_X, 128, 2), stride=(2, 2), **K3)


def case_cin1_xmask(ops):
    return ops.conv_bn_act(_x(1, 8, 8, 1), _w(32, 1), None, _bn(32), act=ACT_LRELU, xmask=torch.ones(1, 1, 1, 8), **K3)


def case_cin1_xmask_out_p16(ops):
    return ops.conv_bn_act(_x(1, 8, 8, 1), _w(32, 1), None, _bn(32), act=ACT_LRELU, xmask=torch.ones(1, 8), out_p16=True, **K3)


def case_xmask_in_front_of_another_layer(ops):
    return _layer(ops, xmask=torch.ones(1, 8))


def case_no_bn_bias_sigmoid(ops):
    return ops.conv_bn_act(_x(*SMALL), _w(32, 32), _b(32), None, act=ACT_SIGMOID, **K3)


def case_eval_bn_bias(ops):
    return ops.conv_bn_act(_x(*SMALL), _w(32, 32), _b(32), _bn(32), act=ACT_RELU, training=False, **K3)


def case_eval_bn_without_running_statistics(ops):
    return ops.conv_bn_act(_x(*SMALL), _w(32, 32), _b(32), _bn(32, track_running_stats=False), act=ACT_RELU, training=False, **K3)


def case_x2_transposed(ops):
    return ops.conv_bn_act(_x(*SMALL), _w(64, 32), None, _bn(32, momentum=None), act=ACT_RELU, x2=_x(*SMALL), transposed=True, **K3)


def case_frames(ops):
    x = torch.zeros(1, 8, 8, 4)                                                   # three channels stored with stride 4
    return ops.conv_bn_act(x, _w(32, 3), None, _bn(32), act=ACT_RELU, **K3)


def case_pair_32(ops):
    return ops.conv_bn_act_cout1(_x(*SMALL), _w(32, 32), None, _bn(32), _w(1, 32), _b(1), act=ACT_RELU, act2=ACT_SIGMOID, **K3)


def case_pair_128(ops):
    return ops.conv_bn_act_cout1(_x(*SMALL), _w(128, 32), _b(128), _bn(128), _w(1, 128), _b(1), act=ACT_LRELU, act2=ACT_SIGMOID, **K3)


def case_pair_direct_grad(ops):
    ops.DIRECT_GRAD = True
    return ops.conv_bn_act_cout1(_x(*SMALL), _w(32, 32, grad=True), None, _bn(32, grad=True), _w(1, 32, grad=True), _b(1, grad=True),
                                 act=ACT_RELU, act2=ACT_SIGMOID, **K3)


def case_direct_grad_all_targets(ops):
    ops.DIRECT_GRAD = True
    return ops.conv_bn_act(_x(*SMALL), _w(32, 32, grad=True), _b(32, grad=True), _bn(32, grad=True), act=ACT_RELU, **K3)


def case_direct_grad_weight_only(ops):
    ops.DIRECT_GRAD = True
    return ops.conv_bn_act(_x(*SMALL), _w(32, 32, grad=True), _b(32), None, act=ACT_RELU, **K3)


CASES = {n[5:]: f for n, f in sorted(globals().items()) if n.startswith("case_")}


def run_case(install, name):
    from viai_amd import ops
    rec = install()
    _back(CASES[name](ops))
    gc.collect()
    return rec


def run_torch_op(install):
    """the plain case through the bodies of torch.ops.viai.conv_bn_act and its backward op (called directly: the dispatcher has no CPU kernel for them)"""
    from viai_amd import torch_ops
    rec = install()
    x, w, bn = torch.zeros(SMALL), _w(32, 32), _bn(32)
    args = ([3, 3], [1, 1], [1, 1], False, ACT_LRELU, True, 0.1, 1e-5)
    with torch.no_grad():
        z, y, coef, xa, _, _ = torch_ops._conv_bn_act._init_fn(x, w, None, bn.weight, bn.bias, bn.running_mean, bn.running_var, *args)
        torch_ops._conv_bn_act_backward._init_fn(torch.ones_like(z), x, w, z, y, coef, xa, False, *args, [True] * 5)
    return rec


# ------------------------------------------------------------------------------------------------------------------- the recorded launches
# What the code answered before the spec existed (one run of this harness on that tree): entry point (without its viai_ prefix), then its
# arguments -- descriptors by name, P for a pointer, 0 for a null one (the stream among them), scalars as passed.
P = "p"
D0 = (1, 8, 8, 1, 0, 32, 3, 3, 1, 1, 1, 1, 0, 1, 1, -1, -1)
D1 = (1, 8, 8, 32, 0, 32, 3, 3, 1, 1, 1, 1, 0, 1, 1, -1, -1)
D2 = (1, 8, 8, 3, 0, 32, 3, 3, 1, 1, 1, 1, 0, 1, 1, -1, -1)
D3 = (1, 8, 8, 32, 0, 128, 3, 3, 1, 1, 1, 1, 0, 1, 1, -1, -1)
D4 = (1, 8, 8, 128, 0, 1, 3, 3, 1, 1, 1, 1, 0, 1, 1, -1, -1)
D5 = (1, 8, 8, 32, 0, 1, 3, 3, 1, 1, 1, 1, 0, 1, 1, -1, -1)
D6 = (1, 128, 128, 32, 0, 32, 3, 3, 1, 1, 1, 1, 0, 1, 1, -1, -1)
D7 = (2, 80, 208, 32, 0, 128, 3, 3, 2, 2, 1, 1, 0, 1, 1, -1, -1)
D8 = (1, 8, 8, 32, 32, 32, 3, 3, 1, 1, 1, 1, 1, 1, 1, -1, -1)
EXPECTED = {
    "cin1_xmask": [
        ("conv2d_pack_fwd", D0, P, P, 0),
        ("conv2d_cin1_bn_fwd", D0, P, P, P, 0, P, 0, 0, 0, 2, 0, 0),
        ("bn_finalize", P, 1, 256, 64, 32, P, P, P, P, P, 0.1, 1e-05, P, P, P, P, 0),
        ("conv2d_cin1_bn_fwd", D0, P, P, P, 0, 0, P, P, P, 2, P, 0),
        ("conv2d_cin1_bn_bwd", D0, P, P, P, 0, P, P, P, P, P, P, P, P, P, P, 2, 1, 0),
        ("conv2d_cin1_bn_wgrad", D0, P, P, P, 0, P, P, P, P, P, P, P, 0, 2, 0),
        ("conv2d_pack_dgrad", D0, P, P, 0),
        ("conv2d_dgrad", D0, P, P, P, 0, 0),
        ("mask_mul", P, P, P, 1, 8, 8, 0),
    ],
    "cin1_xmask_out_p16": [
        ("conv2d_pack_fwd", D0, P, P, 0),
        ("conv2d_cin1_bn_fwd", D0, P, P, P, 0, P, 0, 0, 0, 2, 0, 0),
        ("bn_finalize", P, 1, 256, 64, 32, P, P, P, P, P, 0.1, 1e-05, P, P, P, P, 0),
        ("conv2d_cin1_bn_fwd_p16", D0, P, P, P, 0, P, P, P, P, 64, P, 2, P, 0),
        ("conv2d_cin1_bn_bwd", D0, P, P, P, 0, P, P, P, P, P, P, P, P, P, P, 2, 1, 0),
        ("conv2d_cin1_bn_wgrad", D0, P, P, P, 0, P, P, P, P, P, P, P, 0, 2, 0),
        ("conv2d_pack_dgrad", D0, P, P, 0),
        ("conv2d_dgrad", D0, P, P, P, 0, 0),
        ("mask_mul", P, P, P, 1, 8, 8, 0),
    ],
    "direct_grad_all_targets": [
        ("conv2d_pack_fwd", D1, P, P, 0),
        ("absmax", P, 2048, P, 0),
        ("conv2d_fwd_amax", D1, P, 0, P, P, P, P, 0, P, 0),
        ("bn_finalize", P, 1, 128, 64, 32, P, P, P, P, P, 0.1, 1e-05, P, P, P, P, 0),
        ("bn_act_fwd_amax", P, P, P, P, 64, 32, 1, 0.2, P, 0),
        ("bn_act_bwd_amax", P, P, P, P, P, P, P, P, P, P, P, 64, 32, 1, 0.2, 3, P, 0),
        ("conv2d_wgrad", D1, P, 0, P, P, P, 0, 1, 0),
        ("conv2d_pack_dgrad_f16", D1, P, P, 0),
        ("conv2d_dgrad_f16", D1, P, P, P, 0, P, 0),
    ],
    "direct_grad_weight_only": [
        ("conv2d_pack_fwd", D1, P, P, 0),
        ("absmax", P, 2048, P, 0),
        ("conv2d_fwd_amax", D1, P, 0, P, P, P, 0, 1, P, 0),
        ("act_bwd_from_output", P, P, P, 2048, 1, 0.2, 0),
        ("conv2d_wgrad", D1, P, 0, P, P, P, 0, 1, 0),
        ("colsum", P, 64, 32, P, P, 0, 0),
        ("conv2d_pack_dgrad", D1, P, P, 0),
        ("conv2d_dgrad", D1, P, P, P, 0, 0),
    ],
    "eval_bn_bias": [
        ("conv2d_pack_fwd", D1, P, P, 0),
        ("absmax", P, 2048, P, 0),
        ("conv2d_fwd_amax", D1, P, 0, P, P, P, 0, 0, P, 0),
        ("bn_eval_coeffs", 32, P, P, P, P, 1e-05, P, P, P, P, 0),
        ("bn_act_fwd_amax", P, P, P, P, 64, 32, 1, 0.2, P, 0),
        ("bn_act_bwd_amax", P, P, P, P, P, P, P, P, P, P, P, 64, 32, 1, 0.2, 0, P, 0),
        ("conv2d_wgrad", D1, P, 0, P, P, P, P, 0, 0),
        ("conv2d_pack_dgrad_f16", D1, P, P, 0),
        ("conv2d_dgrad_f16", D1, P, P, P, 0, P, 0),
    ],
    "eval_bn_without_running_statistics": [
        ("conv2d_pack_fwd", D1, P, P, 0),
        ("absmax", P, 2048, P, 0),
        ("conv2d_fwd_amax", D1, P, 0, P, P, P, P, 0, P, 0),
        ("bn_finalize", P, 1, 128, 64, 32, P, P, 0, 0, 0, 0.1, 1e-05, P, P, P, P, 0),
        ("bn_act_fwd_amax", P, P, P, P, 64, 32, 1, 0.2, P, 0),
        ("bn_act_bwd_amax", P, P, P, P, P, P, P, P, P, P, P, 64, 32, 1, 0.2, 1, P, 0),
        ("conv2d_wgrad", D1, P, 0, P, P, P, 0, 0, 0),
        ("conv2d_pack_dgrad_f16", D1, P, P, 0),
        ("conv2d_dgrad_f16", D1, P, P, P, 0, P, 0),
    ],
    "frames": [
        ("conv2d_pack_fwd", D2, P, P, 0),
        ("conv2d_fwd_amax", D2, P, 0, P, 0, P, P, 0, 0, 0),
        ("bn_finalize", P, 1, 128, 64, 32, P, P, P, P, P, 0.1, 1e-05, P, P, P, P, 0),
        ("bn_act_fwd_amax", P, P, P, P, 64, 32, 1, 0.2, P, 0),
        ("bn_act_bwd_amax", P, P, P, P, P, P, P, P, P, P, P, 64, 32, 1, 0.2, 1, 0, 0),
        ("conv2d_wgrad", D2, P, 0, P, P, P, 0, 0, 0),
    ],
    "no_bn_bias_sigmoid": [
        ("conv2d_pack_fwd", D1, P, P, 0),
        ("absmax", P, 2048, P, 0),
        ("conv2d_fwd_amax", D1, P, 0, P, P, P, 0, 3, P, 0),
        ("act_bwd_from_output", P, P, P, 2048, 3, 0.2, 0),
        ("conv2d_wgrad", D1, P, 0, P, P, P, P, 0, 0),
        ("conv2d_pack_dgrad", D1, P, P, 0),
        ("conv2d_dgrad", D1, P, P, P, 0, 0),
    ],
    "pair_128": [
        ("conv2d_pack_fwd", D3, P, P, 0),
        ("conv2d_pack_fwd", D4, P, P, 0),
        ("absmax", P, 2048, P, 0),
        ("conv2d_fwd_amax", D3, P, 0, P, P, P, P, 0, P, 0),
        ("bn_finalize", P, 2, 32, 64, 128, P, P, P, P, P, 0.1, 1e-05, P, P, P, P, 0),
        ("pair_cout1_fwd_dots", D4, P, P, P, 2, P, P, P, P, 3, 0),
        ("act_bwd_from_output", P, P, P, 64, 3, 0.2, 0),
        ("pair_cout1_wgrad", D4, P, P, P, 2, P, P, P, 0, 0),
        ("colsum", P, 64, 1, P, P, 0, 0),
        ("pair_cout1_bn_bwd", D4, P, P, P, P, P, P, P, 2, P, P, P, P, P, 1, P, 0),
        ("conv2d_wgrad", D3, P, 0, P, P, P, 0, 0, 0),
        ("conv2d_pack_dgrad_f16", D3, P, P, 0),
        ("conv2d_dgrad_f16", D3, P, P, P, 0, P, 0),
    ],
    "pair_32": [
        ("conv2d_pack_fwd", D1, P, P, 0),
        ("conv2d_pack_fwd", D5, P, P, 0),
        ("absmax", P, 2048, P, 0),
        ("conv2d_fwd_amax", D1, P, 0, P, 0, P, P, 0, P, 0),
        ("bn_finalize", P, 1, 128, 64, 32, P, P, P, P, P, 0.1, 1e-05, P, P, P, P, 0),
        ("pair_cout1_fwd", D5, P, P, P, 1, P, P, P, 3, 0),
        ("act_bwd_from_output", P, P, P, 64, 3, 0.2, 0),
        ("pair_cout1_wgrad", D5, P, P, P, 1, P, P, P, 0, 0),
        ("colsum", P, 64, 1, P, P, 0, 0),
        ("pair_cout1_bn_bwd", D5, P, P, P, P, P, P, P, 1, P, P, P, P, P, 1, P, 0),
        ("conv2d_wgrad", D1, P, 0, P, P, P, 0, 0, 0),
        ("conv2d_pack_dgrad_f16", D1, P, P, 0),
        ("conv2d_dgrad_f16", D1, P, P, P, 0, P, 0),
    ],
    "pair_direct_grad": [
        ("conv2d_pack_fwd", D1, P, P, 0),
        ("conv2d_pack_fwd", D5, P, P, 0),
        ("absmax", P, 2048, P, 0),
        ("conv2d_fwd_amax", D1, P, 0, P, 0, P, P, 0, P, 0),
        ("bn_finalize", P, 1, 128, 64, 32, P, P, P, P, P, 0.1, 1e-05, P, P, P, P, 0),
        ("pair_cout1_fwd", D5, P, P, P, 1, P, P, P, 3, 0),
        ("act_bwd_from_output", P, P, P, 64, 3, 0.2, 0),
        ("pair_cout1_wgrad", D5, P, P, P, 1, P, P, P, 1, 0),
        ("colsum", P, 64, 1, P, P, 1, 0),
        ("pair_cout1_bn_bwd", D5, P, P, P, P, P, P, P, 1, P, P, P, P, P, 3, P, 0),
        ("conv2d_wgrad", D1, P, 0, P, P, P, 0, 1, 0),
        ("conv2d_pack_dgrad_f16", D1, P, P, 0),
        ("conv2d_dgrad_f16", D1, P, P, P, 0, P, 0),
    ],
    "plain": [
        ("conv2d_pack_fwd", D1, P, P, 0),
        ("absmax", P, 2048, P, 0),
        ("conv2d_fwd_amax", D1, P, 0, P, 0, P, P, 0, P, 0),
        ("bn_finalize", P, 1, 128, 64, 32, P, P, P, P, P, 0.1, 1e-05, P, P, P, P, 0),
        ("bn_act_fwd_amax", P, P, P, P, 64, 32, 2, 0.2, P, 0),
        ("bn_act_bwd_amax", P, P, P, P, P, P, P, P, P, P, P, 64, 32, 2, 0.2, 1, P, 0),
        ("conv2d_wgrad", D1, P, 0, P, P, P, 0, 0, 0),
        ("conv2d_pack_dgrad_f16", D1, P, P, 0),
        ("conv2d_dgrad_f16", D1, P, P, P, 0, P, 0),
    ],
    "plain_out_p16": [
        ("conv2d_pack_fwd", D1, P, P, 0),
        ("absmax", P, 2048, P, 0),
        ("conv2d_fwd_amax", D1, P, 0, P, 0, P, P, 0, P, 0),
        ("bn_finalize", P, 1, 128, 64, 32, P, P, P, P, P, 0.1, 1e-05, P, P, P, P, 0),
        ("bn_act_fwd_p16", P, P, P, P, P, 64, P, 64, 32, 2, 0.2, P, 0),
        ("bn_act_bwd_amax", P, P, P, P, P, P, P, P, P, P, P, 64, 32, 2, 0.2, 1, P, 0),
        ("conv2d_wgrad", D1, P, 0, P, P, P, 0, 0, 0),
        ("conv2d_pack_dgrad_f16", D1, P, P, 0),
        ("conv2d_dgrad_f16", D1, P, P, P, 0, P, 0),
    ],
    "planes_layer": [
        ("conv2d_pack_fwd", D6, P, P, 0),
        ("absmax", P, 524288, P, 0),
        ("conv2d_fwd_amax", D6, P, 0, P, 0, P, P, 0, P, 0),
        ("bn_finalize", P, 128, 128, 16384, 32, P, P, P, P, P, 0.1, 1e-05, P, P, P, P, 0),
        ("bn_act_fwd_p16", P, P, P, P, P, 16384, P, 16384, 32, 1, 0.2, P, 0),
        ("bn_act_bwd_p16", P, P, P, P, P, P, P, P, P, P, P, 16384, 32, 1, 0.2, 1, P, 0),
        ("conv2d_wgrad_f16_p16", D6, P, 0, P, P, P, 0, 0, P, P, 1, 0),
        ("conv2d_pack_dgrad_f16", D6, P, P, 0),
        ("conv2d_dgrad_f16_p16", D6, P, P, P, 0, P, 0),
    ],
    "pool": [
        ("conv2d_pack_fwd", D1, P, P, 0),
        ("absmax", P, 2048, P, 0),
        ("conv2d_fwd_amax", D1, P, 0, P, 0, P, P, 0, P, 0),
        ("bn_finalize", P, 1, 128, 64, 32, P, P, P, P, P, 0.1, 1e-05, P, P, P, P, 0),
        ("bn_act_maxpool_fwd", P, P, P, P, P, 1, 8, 8, 32, 3, 2, 1, 1, 0.2, P, 0),
        ("bn_act_pool_bwd_amax2", P, 0, P, 1, 8, 8, 3, 2, 1, P, P, P, P, P, P, P, P, P, P, 32, 1, 0.2, 1, P, 0),
        ("conv2d_wgrad", D1, P, 0, P, P, P, 0, 0, 0),
        ("conv2d_pack_dgrad_f16", D1, P, P, 0),
        ("conv2d_dgrad_f16", D1, P, P, P, 0, P, 0),
    ],
    "pool_out_p16": [
        ("conv2d_pack_fwd", D1, P, P, 0),
        ("absmax", P, 2048, P, 0),
        ("conv2d_fwd_amax", D1, P, 0, P, 0, P, P, 0, P, 0),
        ("bn_finalize", P, 1, 128, 64, 32, P, P, P, P, P, 0.1, 1e-05, P, P, P, P, 0),
        ("bn_act_maxpool_fwd_twin", P, P, P, P, P, 64, P, P, P, 1, 8, 8, 32, 3, 2, 1, 1, 0.2, P, P, 0),
        ("bn_act_pool_bwd_amax2", P, 0, P, 1, 8, 8, 3, 2, 1, P, P, P, P, P, P, P, P, P, P, 32, 1, 0.2, 1, P, 0),
        ("conv2d_wgrad", D1, P, 0, P, P, P, 0, 0, 0),
        ("conv2d_pack_dgrad_f16", D1, P, P, 0),
        ("conv2d_dgrad_f16", D1, P, P, P, 0, P, 0),
    ],
    "res": [
        ("conv2d_pack_fwd", D1, P, P, 0),
        ("absmax", P, 2048, P, 0),
        ("conv2d_fwd_amax", D1, P, 0, P, 0, P, P, 0, P, 0),
        ("bn_finalize", P, 1, 128, 64, 32, P, P, P, P, P, 0.1, 1e-05, P, P, P, P, 0),
        ("bn_add_act_fwd_amax", P, P, P, P, P, 64, 32, 1, 0.2, P, 0),
        ("act_bwd_from_output", P, P, P, 2048, 1, 0.2, 0),
        ("bn_act_bwd_amax", P, P, P, P, P, P, P, P, P, P, P, 64, 32, 0, 0.2, 1, P, 0),
        ("conv2d_wgrad", D1, P, 0, P, P, P, 0, 0, 0),
        ("conv2d_pack_dgrad_f16", D1, P, P, 0),
        ("conv2d_dgrad_f16", D1, P, P, P, 0, P, 0),
    ],
    "res_out_p16": [
        ("conv2d_pack_fwd", D1, P, P, 0),
        ("absmax", P, 2048, P, 0),
        ("conv2d_fwd_amax", D1, P, 0, P, 0, P, P, 0, P, 0),
        ("bn_finalize", P, 1, 128, 64, 32, P, P, P, P, P, 0.1, 1e-05, P, P, P, P, 0),
        ("bn_add_act_fwd_twin", P, P, P, P, P, 64, P, P, P, P, 64, 32, 1, 0.2, P, P, 0),
        ("act_bwd_from_output", P, P, P, 2048, 1, 0.2, 0),
        ("bn_act_bwd_amax", P, P, P, P, P, P, P, P, P, P, P, 64, 32, 0, 0.2, 1, P, 0),
        ("conv2d_wgrad", D1, P, 0, P, P, P, 0, 0, 0),
        ("conv2d_pack_dgrad_f16", D1, P, P, 0),
        ("conv2d_dgrad_f16", D1, P, P, P, 0, P, 0),
    ],
    "res_twin_consumed": [
        ("conv2d_pack_fwd", D6, P, P, 0),
        ("conv2d_fwd_p16", D6, P, P, 0, P, P, 0, P, 0),
        ("bn_finalize", P, 128, 128, 16384, 32, P, P, P, P, P, 0.1, 1e-05, P, P, P, P, 0),
        ("bn_add_act_fwd_twin", P, P, P, P, P, 16384, P, P, P, P, 16384, 32, 1, 0.2, P, P, 0),
        ("bn_join_bwd_p16", P, 0, P, P, P, P, P, P, P, P, P, P, P, P, 16384, 32, 1, P, 0),
        ("conv2d_wgrad_f16_p16", D6, P, 0, P, P, P, 0, 0, P, P, 3, 0),
        ("conv2d_pack_dgrad_f16", D6, P, P, 0),
        ("conv2d_dgrad_f16_p16", D6, P, P, P, 0, P, 0),
    ],
    "res_twin_for_the_weight_gradient": [
        ("conv2d_pack_fwd", D7, P, P, 0),
        ("conv2d_fwd_amax", D7, P, 0, P, 0, P, P, 0, P, 0),
        ("bn_finalize", P, 260, 32, 8320, 128, P, P, P, P, P, 0.1, 1e-05, P, P, P, P, 0),
        ("bn_add_act_fwd_amax", P, P, P, P, P, 8320, 128, 1, 0.2, P, 0),
        ("act_bwd_from_output", P, P, P, 1064960, 1, 0.2, 0),
        ("bn_act_bwd_p16_twin", P, P, P, P, P, P, P, P, P, P, P, P, 8320, 128, 0, 0.2, 1, P, 0),
        ("conv2d_wgrad_f16_p16", D7, P, 0, P, P, P, 0, 0, P, P, 3, 0),
        ("conv2d_pack_dgrad_f16", D7, P, P, 0),
        ("conv2d_dgrad_f16", D7, P, P, P, 0, P, 0),
    ],
    "up": [
        ("conv2d_pack_fwd", D1, P, P, 0),
        ("absmax", P, 2048, P, 0),
        ("conv2d_fwd_amax", D1, P, 0, P, 0, P, P, 0, P, 0),
        ("bn_finalize", P, 1, 128, 64, 32, P, P, P, P, P, 0.1, 1e-05, P, P, P, P, 0),
        ("bn_act_bilinear_fwd_amax", P, P, P, P, 1, 8, 8, 16, 16, 32, 1, 0.2, P, 0),
        ("bilinear_ac_bwd", P, P, 1, 8, 8, 16, 16, 32, 0),
        ("bn_act_bwd_amax", P, P, P, P, P, P, P, P, P, P, P, 64, 32, 1, 0.2, 1, P, 0),
        ("conv2d_wgrad", D1, P, 0, P, P, P, 0, 0, 0),
        ("conv2d_pack_dgrad_f16", D1, P, P, 0),
        ("conv2d_dgrad_f16", D1, P, P, P, 0, P, 0),
    ],
    "up_out_p16": [
        ("conv2d_pack_fwd", D1, P, P, 0),
        ("absmax", P, 2048, P, 0),
        ("conv2d_fwd_amax", D1, P, 0, P, 0, P, P, 0, P, 0),
        ("bn_finalize", P, 1, 128, 64, 32, P, P, P, P, P, 0.1, 1e-05, P, P, P, P, 0),
        ("bn_act_bilinear_fwd_p16", P, P, P, P, P, 64, P, 1, 8, 8, 16, 16, 32, 1, 0.2, P, 0),
        ("bilinear_ac_bwd", P, P, 1, 8, 8, 16, 16, 32, 0),
        ("bn_act_bwd_amax", P, P, P, P, P, P, P, P, P, P, P, 64, 32, 1, 0.2, 1, P, 0),
        ("conv2d_wgrad", D1, P, 0, P, P, P, 0, 0, 0),
        ("conv2d_pack_dgrad_f16", D1, P, P, 0),
        ("conv2d_dgrad_f16", D1, P, P, P, 0, P, 0),
    ],
    "x2_transposed": [
        ("conv2d_pack_fwd", D8, P, P, 0),
        ("absmax", P, 2048, P, 0),
        ("absmax", P, 2048, P, 0),
        ("conv2d_fwd_amax", D8, P, P, P, 0, P, P, 0, P, 0),
        ("bn_finalize", P, 1, 128, 64, 32, P, P, P, P, P, 0.1, 1e-05, P, P, P, P, 0),
        ("bn_act_fwd_amax", P, P, P, P, 64, 32, 1, 0.2, P, 0),
        ("bn_act_bwd_amax", P, P, P, P, P, P, P, P, P, P, P, 64, 32, 1, 0.2, 1, P, 0),
        ("conv2d_wgrad", D8, P, P, P, P, P, 0, 0, 0),
        ("conv2d_pack_dgrad_f16", D8, P, P, 0),
        ("conv2d_dgrad_f16", D8, P, P, P, P, P, 0),
    ],
    "xmask_in_front_of_another_layer": [
        ("mask_mul", P, P, P, 1, 256, 8, 0),
        ("conv2d_pack_fwd", D1, P, P, 0),
        ("absmax", P, 2048, P, 0),
        ("conv2d_fwd_amax", D1, P, 0, P, 0, P, P, 0, P, 0),
        ("bn_finalize", P, 1, 128, 64, 32, P, P, P, P, P, 0.1, 1e-05, P, P, P, P, 0),
        ("bn_act_fwd_amax", P, P, P, P, 64, 32, 1, 0.2, P, 0),
        ("bn_act_bwd_amax", P, P, P, P, P, P, P, P, P, P, P, 64, 32, 1, 0.2, 1, P, 0),
        ("conv2d_wgrad", D1, P, 0, P, P, P, 0, 0, 0),
        ("conv2d_pack_dgrad_f16", D1, P, P, 0),
        ("conv2d_dgrad_f16", D1, P, P, P, 0, P, 0),
        ("mask_mul", P, P, P, 1, 256, 8, 0),
    ],
    "torch_op_plain": [
        ("conv2d_pack_fwd", D1, P, P, 0),
        ("absmax", P, 2048, P, 0),
        ("conv2d_fwd_amax", D1, P, 0, P, 0, P, P, 0, P, 0),
        ("bn_finalize", P, 1, 128, 64, 32, P, P, P, P, 0, 0.1, 1e-05, P, P, P, P, 0),
        ("bn_act_fwd_amax", P, P, P, P, 64, 32, 2, 0.2, P, 0),
        ("bn_act_bwd_amax", P, P, P, P, P, P, P, P, P, P, P, 64, 32, 2, 0.2, 1, P, 0),
        ("conv2d_wgrad", D1, P, 0, P, P, P, 0, 0, 0),
        ("conv2d_pack_dgrad_f16", D1, P, P, 0),
        ("conv2d_dgrad_f16", D1, P, P, P, 0, P, 0),
    ],
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_launch_sequence_is_the_recorded_one(harness, name):
    rec = run_case(harness, name)
    assert [(n[5:],) + args for n, args in scalars(rec.log)] == EXPECTED[name]


def test_registered_op_launches_what_conv_bn_act_launches(harness):
    """torch.ops.viai.conv_bn_act beside ops.conv_bn_act on the plain layer: the same calls with the same scalars (the functional op hands the kernels
    no batch counter, so one pointer of viai_bn_finalize is null there: pointers are left out of this comparison, and pinned by the record)"""
    op = run_torch_op(harness)
    assert [(n[5:],) + args for n, args in scalars(op.log)] == EXPECTED["torch_op_plain"]
    assert scalars(op.log, nullness=False) == scalars(run_case(harness, "plain").log, nullness=False)


def test_spec_is_kept_and_never_written(harness):
    """ctx.state holds the spec the builder made, and forward and backward leave every field as it was"""
    from viai_amd import ops
    made = []
    build = ops._layer_spec

    def spy(*a, **kw):
        made.append(build(*a, **kw)[0])
        return made[-1], build(*a, **kw)[1]
    for name in sorted(CASES):
        harness()
        del made[:]
        ops._layer_spec = spy
        try:
            z = CASES[name](ops)
        finally:
            ops._layer_spec = build
        spec = z.grad_fn.state.spec
        assert spec is made[0] or (name == "xmask_in_front_of_another_layer" and spec == made[0]._replace(xmask=None)), name
        fields = tuple(spec)
        _back(z)
        assert z.grad_fn.state.spec is spec and len(fields) == len(ops._LayerSpec._fields), name
        assert all(a is b or a == b for a, b in zip(fields, spec)), name
        ops.DIRECT_GRAD = False


def test_twin_outlives_the_forward_only_where_a_kernel_still_reads_it(harness):
    """a pre-split copy beside x: kept behind the forward as the saved x (the forward read the planes) or as x_twin_w (only the weight gradient
    stages pieces), released with the caller's reference where the layer has no use for it; gone after the backward in every case"""
    from viai_amd import ops
    for shape, cout, stride, kept in ((PLANES, 32, 1, True), (WGRAD_X, 128, 2, True), (SMALL, 32, 1, False)):
        harness()
        x = _with_twin(_x(*shape))
        ref = weakref.ref(x._viai_twin)
        z = ops.conv_bn_act(x, _w(cout, 32), None, _bn(cout), act=ACT_RELU, stride=(stride, stride), **K3)
        assert (z.grad_fn.state.x_twin_w is not None) == (shape == WGRAD_X)
        del x._viai_twin
        gc.collect()
        assert (ref() is not None) == kept, shape
        _back(z)
        del z
        gc.collect()
        assert ref() is None, shape
