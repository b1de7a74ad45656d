"""The host path of WaveNet synthesis (viai_amd/wavenet_synth.py), pinned without a GPU.  Nothing is launched: `_lib.load` hands out a recording
stub that answers the host queries from the real library (it loads without a device), fakes `viai_wn_pipe_ok` and the three launch entry points,
and reads the descriptor each launch is handed.  The networks are built without weight normalisation and without the conditioning up-sampler, on CPU
tensors, so no set-up kernel is needed either.

  * `_synth_form` over its whole input space against the expressions it replaced, written out below as they stood.
  * the descriptor: every scalar field, and the bytes behind every weight pointer against the rearranged module parameters.
  * the input forms of the one-hot network, the launch sequences of the chain and pipelined runners, the device error of the pipelined one.
  * set-up launches: one weight-norm call per holder module.
"""
import ctypes as C
import itertools
import math
import os

import numpy as np
import pytest
import torch

BOOLS = (False, True)


@pytest.fixture(scope="module")
def real_lib():
    from viai_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def _read(ptr, n, ctype=C.c_float):
    return None if not ptr else np.ctypeslib.as_array((ctype * n).from_address(ptr)).copy()


class Recorder:
    """stands in for the loaded library: `calls` is the ordered list of launches, `desc` what the first launch's descriptor held"""

    def __init__(self, real, pipe_ok=0, err=(0, 0, 0, 0)):
        self.real, self.pipe_ok, self.err, self.calls, self.desc = real, pipe_ok, err, [], None
        for n in ("viai_wn_categorical_ok", "viai_wn_pipe_image_floats", "viai_wn_pipe_token_granules"):
            setattr(self, n, getattr(real, n))

    def viai_wn_pipe_ok(self, ref):
        return self.pipe_ok

    def _launch(self, name, ref, *args):
        self.calls.append((name,) + args)
        if self.desc is None:
            self.desc = snapshot(ref._obj)
        return 0

    def viai_wavenet_synth_run(self, ref, t0, n, stream):
        return self._launch("viai_wavenet_synth_run", ref, t0, n)

    def viai_wavenet_synth_step(self, ref, stream):
        return self._launch("viai_wavenet_synth_step", ref)

    def viai_wn_pipe_run(self, ref, i0, i1, i2, i3, i4, i5, tok, err, t0, n, stream):
        assert all((i0, i1, i2, i3, i4, i5, tok, err))
        (C.c_int32 * 4).from_address(err)[:] = self.err
        return self._launch("viai_wn_pipe_run", ref, t0, n)


def snapshot(st):
    """scalars of a `WnSynth` and copies of what its weight and input pointers point to (sizes from its own dimensions)"""
    B, Cc, G, S, K, H = st.B, st.C, st.G, st.S, st.out_ch, st.G // 2
    kin = K if st.categorical else 1
    d = {n: getattr(st, n) for n in ("B", "C", "G", "S", "cin", "n_layers", "out_ch", "T", "n_test", "log_scale_min", "fused", "categorical",
                                     "cat_softmax", "cat_quantize", "init_class")}
    sizes = {"w_first": Cc * kin, "b_first": Cc, "w_first_t": K * Cc, "w_l1": S * S, "b_l1": S, "w_l2": K * S, "b_l2": K,
             "test_inputs": B * st.n_test * kin, "init_rows": B * K}
    for n, size in sizes.items():
        d[n] = _read(getattr(st, n), size)
    d["test_classes"] = _read(st.test_classes, B * st.n_test, C.c_int32)
    d["nonnull"] = {n for n in ("cond", "u1", "u2", "out", "z", "z2", "skips", "step", "yhat_dbg", "classes") if getattr(st, n)}
    d["layers"] = []
    for l in range(st.n_layers):
        L = st.layers[l]
        sizes = {"w_conv": G * 3 * Cc, "b_conv": G, "w_c": G * st.cin, "b_c": G, "w_out": Cc * H, "b_out": Cc, "w_skip": S * H, "b_skip": S,
                 "w_stage": G * (3 * Cc + (H if l else 0)), "b_stage": G}
        e = {n: _read(getattr(L, n), size) for n, size in sizes.items()}
        e.update(dilation=L.dilation, ring_len=L.ring_len, ring=bool(L.ring), g_add=bool(L.g_add))
        d["layers"].append(e)
    return d


@pytest.fixture
def harness(monkeypatch, real_lib):
    """incremental_forward without a device: returns a function that installs a Recorder with the given answers"""
    from viai_amd import _lib, ops, wavenet_synth

    class _NoStream:
        def synchronize(self):
            pass
    monkeypatch.setattr(wavenet_synth, "_stream", lambda: 0)
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a: _NoStream())
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: None)
    monkeypatch.delenv("VIAI_WN_FUSED", raising=False)
    monkeypatch.delenv("VIAI_WN_PIPE", raising=False)

    def install(**kw):
        rec = Recorder(real_lib, **kw)
        monkeypatch.setattr(_lib, "load", lambda: rec)
        return rec
    return install


def make_net(onehot=False, cin=4, layers=4, stacks=2, weight_normalization=False):
    from viai_amd.wavenet import WaveNet
    torch.manual_seed(5)
    net = WaveNet(out_channels=8 if onehot else 30, layers=layers, stacks=stacks, residual_channels=8, gate_channels=8, skip_out_channels=8,
                  cin_channels=cin, upsample_conditional_features=False, scalar_input=not onehot, weight_normalization=weight_normalization).eval()
    if not weight_normalization:
        for p in net.parameters():                                      # (biases start at zero: make every buffer tell)
            p.data.uniform_(-0.5, 0.5)
    return net


def one_hot_rows(B, n, K=8):
    cls = (torch.arange(B * n).reshape(B, n) * 3 + 1) % K
    return cls, torch.nn.functional.one_hot(cls, K).float()              # (B, n), (B, n, K)


# ----------------------------------------------------------------------------- _synth_form
def spec_form(use_graph, fuse, pipe_env, pipe_ok, categorical_ok, cat, B, T):
    """WaveNet.incremental_forward before wavenet_synth._synth_form: the `pipe` expression, the two NotImplementedErrors in their order, the
    if / elif / else over the three runners"""
    pipe = (not use_graph) and fuse and pipe_env and bool(pipe_ok)
    if not pipe and B not in (1, 2, 4, 8):
        raise NotImplementedError("incremental_forward: the chain of launches takes 1, 2, 4 or 8 streams; any other count up to 32 needs the pipelined form "
                                  "(reference-size network, local conditioning only, no use_graph, VIAI_WN_PIPE != 0, a device with 256 compute units)")
    if cat and not categorical_ok:
        raise NotImplementedError("incremental_forward: the one-hot network needs out_channels <= 256 and a multiple of 4, channel counts that are multiples of 4")
    if pipe:
        return "pipe"
    elif use_graph and T > 2:
        return "graph"
    else:
        return "chain"


def test_synth_form_agrees_with_the_expressions_it_replaced_on_every_input():
    from viai_amd.wavenet_synth import _synth_form

    def outcome(fn, args):
        try:
            return fn(*args)
        except Exception as e:
            return type(e), str(e)
    seen = set()
    for args in itertools.product(BOOLS, BOOLS, BOOLS, BOOLS, BOOLS, BOOLS, range(34), (1, 2, 3, 100)):
        want = outcome(spec_form, args)
        assert outcome(_synth_form, args) == want, args
        seen.add(want if isinstance(want, str) else want[0])
    assert seen == {"pipe", "graph", "chain", NotImplementedError}


# ----------------------------------------------------------------------------- descriptor contents
def _lin(m):
    return m.weight.detach().permute(0, 2, 1).reshape(m.weight.size(0), -1).contiguous()


def spec_stage_rows(net, cond_on):
    """the fused stages' extended gate rows [Wc^0 | Wc^1 | r Wc^2 | r Wc^2 Wo_prev] and bias b + b_c + r Wc^2 bo_prev, in fp64, rounded once
    to fp32.  The same torch fp64 operations in the same order as the host path, so the comparison is bitwise."""
    r5, Cc, prev, rows = math.sqrt(0.5), net.first_conv.bias.numel(), None, []
    for f in net.conv_layers:
        w, b = _lin(f.conv).double(), f.conv.bias.detach().double()
        if cond_on and f.conv1x1c is not None:
            b = b + f.conv1x1c.bias.detach().double()
        if prev is not None:
            w2 = w[:, 2 * Cc:]
            wo = prev.conv1x1_out.weight.detach().reshape(Cc, -1).double()
            w = torch.cat((w[:, :2 * Cc], r5 * w2, r5 * (w2 @ wo)), 1)
            b = b + r5 * (w2 @ prev.conv1x1_out.bias.detach().double())
        rows.append((w.float().numpy().reshape(-1), b.float().numpy()))
        prev = f
    return rows


def same_bits(got, want):
    want = np.ascontiguousarray(want.detach().numpy() if torch.is_tensor(want) else want, dtype=np.float32).reshape(-1)
    return got is not None and got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("cond", ["off", "unused", "on"])             # no conv1x1c; conv1x1c there but no c given; c given
@pytest.mark.parametrize("onehot", BOOLS)
def test_descriptor_contents(harness, monkeypatch, onehot, cond, fused):
    monkeypatch.setenv("VIAI_WN_FUSED", str(fused))
    rec = harness()
    net = make_net(onehot, cin=-1 if cond == "off" else 4)
    B, T, K = 2, 6, net.out_channels
    c = torch.rand(B, 4, T) if cond == "on" else None
    if onehot:
        init = torch.rand(B, K, 1)
        out = net.incremental_forward(init, c=c, T=T, uniforms=torch.rand(B, T))
        assert tuple(out.shape) == (B, K, T)
    else:
        tin = torch.rand(B, 1, 3)
        out = net.incremental_forward(None, c=c, T=T, test_inputs=tin, uniforms=(torch.rand(B, T, 10), torch.rand(B, T)), log_scale_min=-6.5)
        assert tuple(out.shape) == (B, 1, T)
    d = rec.desc
    want = dict(B=B, C=8, G=8, S=8, cin=4, n_layers=4, out_ch=K, T=T, n_test=0 if onehot else 3, log_scale_min=-7.0 if onehot else -6.5, fused=fused,
                categorical=int(onehot), cat_softmax=int(onehot), cat_quantize=int(onehot), init_class=0)
    assert {k: d[k] for k in want} == want
    assert d["nonnull"] == {"u2", "out", "z", "z2", "skips", "step"} | ({"classes", "yhat_dbg"} if onehot else {"u1"}) | ({"cond"} if c is not None else set())
    first = net.first_conv.weight.detach().reshape(8, -1)
    assert same_bits(d["w_first"], first) and same_bits(d["b_first"], net.first_conv.bias)
    assert same_bits(d["w_first_t"], first.t()) if onehot else d["w_first_t"] is None
    l1, l2 = net.last_conv_layers[1], net.last_conv_layers[3]
    assert same_bits(d["w_l1"], l1.weight) and same_bits(d["b_l1"], l1.bias) and same_bits(d["w_l2"], l2.weight) and same_bits(d["b_l2"], l2.bias)
    if onehot:
        assert same_bits(d["init_rows"], init.reshape(B, K)) and d["test_inputs"] is None and d["test_classes"] is None
    else:
        assert same_bits(d["test_inputs"], tin) and d["init_rows"] is None
    stage = spec_stage_rows(net, c is not None)
    for l, (f, e) in enumerate(zip(net.conv_layers, d["layers"])):
        assert (e["dilation"], e["ring_len"], e["ring"], e["g_add"]) == (2 ** (l % 2), 2 * 2 ** (l % 2) + 1, True, False)
        assert same_bits(e["w_conv"], _lin(f.conv)) and same_bits(e["b_conv"], f.conv.bias)
        assert same_bits(e["w_out"], f.conv1x1_out.weight) and same_bits(e["b_out"], f.conv1x1_out.bias)
        assert same_bits(e["w_skip"], f.conv1x1_skip.weight) and same_bits(e["b_skip"], f.conv1x1_skip.bias)
        if c is not None:
            assert same_bits(e["w_c"], f.conv1x1c.weight) and same_bits(e["b_c"], f.conv1x1c.bias)
        else:
            assert e["w_c"] is None and e["b_c"] is None
        if fused:
            assert same_bits(e["w_stage"], stage[l][0]) and same_bits(e["b_stage"], stage[l][1])
        else:
            assert e["w_stage"] is None and e["b_stage"] is None


# ----------------------------------------------------------------------------- one-hot input forms
def test_onehot_input_forms(harness):
    net = make_net(onehot=True)
    B, n, K = 2, 5, 8
    cls, rows = one_hot_rows(B, n)

    def run(x, **kw):
        rec = harness()
        net.incremental_forward(None, T=n, test_inputs=x, uniforms=torch.rand(B, n), **kw)
        return rec.desc
    a, b = run(rows), run(rows.transpose(1, 2).contiguous())                     # (B, n, K) and (B, K, n)
    assert a["n_test"] == b["n_test"] == n and same_bits(a["test_inputs"], rows) and same_bits(b["test_inputs"], rows)
    assert np.array_equal(a["test_classes"], cls.numpy().reshape(-1)) and np.array_equal(b["test_classes"], cls.numpy().reshape(-1))
    assert run(rows, input_form="dense")["test_classes"] is None
    soft = rows.clone()
    soft[1, 2] = 0
    soft[1, 2, :2] = 0.5
    d = run(soft)
    assert d["test_classes"] is None and same_bits(d["test_inputs"], soft)


# ----------------------------------------------------------------------------- launch sequences
@pytest.mark.parametrize("onehot", BOOLS)
def test_chain_launch_sequence(harness, onehot):
    net = make_net(onehot)
    init = torch.rand(1, 8, 1) if onehot else None
    rec, timing = harness(), {"warmup": 3}
    net.incremental_forward(init, T=150, timing=timing)
    assert rec.calls == [("viai_wavenet_synth_run",) + p for p in ((0, 3), (3, 64), (67, 64), (131, 19))]
    assert timing["steps"] == 147 and timing["ms"] >= 0 and "form" not in timing
    rec = harness()
    net.incremental_forward(init, T=150)
    assert rec.calls == [("viai_wavenet_synth_run",) + p for p in ((0, 64), (64, 64), (128, 22))]


def _zero_images(real_lib):
    n = [real_lib.viai_wn_pipe_image_floats(k) for k in range(6)]
    return lambda *a: tuple(torch.zeros(n[k]) for k in (0, 5, 1, 2, 3, 4))         # wreg, wcond, wlds, bias, head_w, head_b


def test_pipe_launch_sequence_and_device_error(harness, monkeypatch, real_lib):
    from viai_amd import _lib, wavenet_synth
    monkeypatch.setattr(wavenet_synth, "_pipe_images", _zero_images(real_lib))
    net = make_net(layers=24, stacks=4)                                          # the token-ring query reads 24 dilations
    rec, timing = harness(pipe_ok=1), {"warmup": 100}
    net.incremental_forward(None, T=2500, timing=timing)
    assert rec.calls == [("viai_wn_pipe_run",) + p for p in ((0, 100), (100, 1024), (1124, 1024), (2148, 352))]
    assert timing["form"] == "pipe" and timing["steps"] == 2400
    rec = harness(pipe_ok=1, err=(1, 7, 0, 41))
    with pytest.raises(_lib.ViaiLibraryError) as ei:
        net.incremental_forward(None, T=8)
    assert str(ei.value) == ("viai_wn_pipe_run failed on the device: a wait timed out at stage 7, stream 0, t = 41 (the pipelined form needs all of its 249 "
                             "blocks resident at once, i.e. the whole chip to itself; VIAI_WN_PIPE=0 selects the chain of launches)")
    rec = harness(pipe_ok=1)                                                     # use_graph and VIAI_WN_PIPE=0 keep the chain forms
    monkeypatch.setenv("VIAI_WN_PIPE", "0")
    net.incremental_forward(None, T=8)
    assert rec.calls == [("viai_wavenet_synth_run", 0, 8)]


# ----------------------------------------------------------------------------- set-up launches
@pytest.mark.parametrize("onehot,cond,pipe", [(False, False, 0), (False, True, 0), (True, True, 0), (False, True, 1)])
def test_one_weight_norm_launch_per_holder_module(harness, monkeypatch, real_lib, onehot, cond, pipe):
    from viai_amd import wavenet, wavenet_synth
    seen = []

    def identity(v, g):
        seen.append(v)
        return v
    monkeypatch.setattr(wavenet._WeightNorm, "apply", staticmethod(identity))
    monkeypatch.setattr(wavenet_synth, "_pipe_images", _zero_images(real_lib))
    net = make_net(onehot, layers=24, stacks=4, weight_normalization=True)
    rec = harness(pipe_ok=pipe)
    net.incremental_forward(torch.rand(1, 8, 1) if onehot else None, c=torch.rand(1, 4, 4) if cond else None, T=4)
    assert rec.calls[0][0] == ("viai_wn_pipe_run" if pipe else "viai_wavenet_synth_run")
    holders = [net.first_conv, net.last_conv_layers[1], net.last_conv_layers[3]]
    for f in net.conv_layers:
        holders += [f.conv, f.conv1x1_out, f.conv1x1_skip] + ([f.conv1x1c] if cond else [])
    assert sorted(id(v) for v in seen) == sorted(id(m.weight_v) for m in holders)
