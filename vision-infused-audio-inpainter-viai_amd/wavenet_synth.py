"""Host path of `WaveNet.incremental_forward` (sample-by-sample synthesis, wavenet.py:237-364 of the reference), in the order a call goes through it:

  _resolve_inputs   argument checks, normalised inputs, the mask of forced steps, conditioning up-sample, the sampler's uniforms -> _Inputs
  _synth_weights    every holder module's effective weight, once, in every layout the launch forms read    -> _Weights
  _SynthState       owns every tensor the C descriptor (`_lib.WnSynth` / `_lib.WnLayer`) points to, and builds the descriptor
  _synth_form       which launch form runs: "pipe" (csrc/wavenet_pipe.hip), "graph" or "chain" (csrc/wavenet.hip) -- a pure function; a call with a
                    mask of forced steps takes the chain forms (the pipelined kernel knows the prefix rule only)
  _run_pipe / _run_graph / _run_chain

The kernels, the descriptor's layout and the arithmetic of a time step are described in include/viai_hip.h and DESIGN.md 11.2 / 11.2b.
"""
from __future__ import annotations

import ctypes as Ct
import math
import os
import time
from collections import namedtuple

import torch

from . import _lib, wavenet as W
from .ops import _ptr, _stream

_Inputs = namedtuple("_Inputs", "B T tin tcls init_rows cond u1 u2 g_vec forced")
# per layer (lists): w_conv .. b_stage; w_c / b_c hold None without conditioning, w_stage / b_stage without the fused stages.  w_first_t: one-hot network only.
_LAYER_FIELDS = ("w_conv", "b_conv", "w_c", "b_c", "w_out", "b_out", "w_skip", "b_skip", "w_stage", "b_stage")          # of `_lib.WnLayer`: a list each
_NET_FIELDS = ("w_first", "b_first", "w_first_t", "w_l1", "b_l1", "w_l2", "b_l2")                                       # of `_lib.WnSynth`
_Weights = namedtuple("_Weights", _LAYER_FIELDS + _NET_FIELDS)


def _resolve_inputs(net, initial_input, c, g, T, test_inputs, softmax, quantize, uniforms, return_logits, return_classes, input_form, forced=None,
                    c_upsampled=False):
    """The checks of the arguments (the one-hot network's four and the mask's come first: nothing has touched the library or the device by then)
    and the inputs as the kernels read them: tin (B, n, K) / (B, n), tcls (B, n) int32 where the teacher-forced rows are exactly one-hot (or were
    given as integer classes), init_rows (B, K), cond (B, T, cin), the uniforms u1 (B, T, 10) / u2 (B, T), g_vec (B, gin, 1), forced (B, T) uint8.
    With `forced` the number of steps is the mask's and test_inputs must have exactly that length; rows the mask does not force are never read."""
    cat, K = not net.scalar_input, net.out_channels
    if forced is not None:
        if test_inputs is None:
            raise ValueError("incremental_forward: forced= marks which steps of test_inputs are used; it needs test_inputs")
        if forced.dim() != 2 or forced.dtype not in (torch.bool, torch.uint8):
            raise ValueError("incremental_forward: forced is a (B, T) bool or uint8 tensor")
    if cat:
        if quantize and not softmax:
            raise ValueError("incremental_forward: quantize=True needs softmax=True (logits are no probabilities to draw a class from)")
        if return_logits:
            raise ValueError("incremental_forward: return_logits belongs to the mixture-of-logistics network; softmax=False, quantize=False returns the logits")
        if return_classes and not quantize:
            raise ValueError("incremental_forward: return_classes needs quantize=True")
        if input_form not in ("auto", "dense"):
            raise ValueError("incremental_forward: input_form is 'auto' or 'dense'")
    dev = net.first_conv.bias.device
    tin = tcls = init_rows = None
    if test_inputs is not None:
        as_classes = cat and test_inputs.dim() == 2 and not torch.is_floating_point(test_inputs)      # (B, n) integer classes: no one-hot tensor
        if as_classes and input_form == "dense":
            raise ValueError("incremental_forward: integer classes as test_inputs have no dense form")
        if not as_classes and test_inputs.size(1) == (K if cat else 1):
            test_inputs = test_inputs.transpose(1, 2)                                 # -> (B, n, K) / (B, n, 1)  (wavenet.py:268-274)
        B = test_inputs.size(0)
        if forced is not None:
            if forced.size(0) != B:
                raise ValueError("incremental_forward: forced is (B, T); it has %d rows, test_inputs %d streams" % (forced.size(0), B))
            if test_inputs.size(1) != forced.size(1):
                raise ValueError("incremental_forward: forced covers %d steps, test_inputs %d; a mask needs test_inputs of exactly its length"
                                 % (forced.size(1), test_inputs.size(1)))
            T = forced.size(1)
            forced = forced.to(dev).to(torch.uint8).contiguous()
        T = test_inputs.size(1) if T is None else max(int(T), test_inputs.size(1))
        if as_classes:
            tcls = test_inputs.to(dev).to(torch.int32).contiguous()
        elif cat:
            tin = test_inputs.to(dev).float().contiguous()                            # (B, n, K)
            assert tin.size(2) == K, "test_inputs: (B, K, n) or (B, n, K)"
            hot = ((tin == 0) | (tin == 1)).all(-1) & (tin.sum(-1) == 1)
            if forced is not None:
                hot = hot | (forced == 0)                                             # rows the mask does not force may hold anything
            if input_form == "auto" and bool(hot.all()):
                tcls = tin.argmax(-1).to(torch.int32).contiguous()                    # exactly one-hot rows: the class form
        else:
            tin = test_inputs.reshape(B, -1).to(dev).float().contiguous()
    else:
        B = c.size(0) if c is not None else (initial_input.size(0) if (cat and initial_input is not None) else 1)
    T = int(T)
    if cat and initial_input is None and tin is None and tcls is None and K <= 127:
        raise ValueError("incremental_forward: the default initial input is class 127 (wavenet.py:308-312); with %d classes pass initial_input" % K)
    if cat and initial_input is not None:                                             # wavenet.py:316-318
        if initial_input.size(1) == K:
            initial_input = initial_input.transpose(1, 2)
        init_rows = initial_input.to(dev).float().reshape(B, K).contiguous()
    if not 1 <= B <= 32:
        raise NotImplementedError("incremental_forward: 1 to 32 streams")
    cond = None
    if c is not None:
        cu = c.to(dev).float() if c_upsampled else net._upsample(c.to(dev).float())
        assert cu.size(-1) == T
        cond = cu.transpose(1, 2).contiguous()                                        # (B, T, cin)
    if cat:
        u1 = None
        u2 = torch.rand(B, T, device=dev) if uniforms is None else uniforms.to(dev).float().reshape(B, T).contiguous()
    elif uniforms is None:
        u1 = torch.empty(B, T, K // 3, device=dev).uniform_(1e-5, 1.0 - 1e-5)
        u2 = torch.empty(B, T, device=dev).uniform_(1e-5, 1.0 - 1e-5)
    else:
        u1, u2 = uniforms[0].to(dev).float().contiguous(), uniforms[1].to(dev).float().contiguous()
    g_vec = None
    if g is not None:                                                                # wavenet.py:284-290: time-invariant
        g = g.to(dev)
        g_vec = (net.embed_speakers(g.view(B, -1)).transpose(1, 2) if net.embed_speakers is not None else g.float().view(B, -1, 1)).contiguous()
    return _Inputs(B, T, tin, tcls, init_rows, cond, u1, u2, g_vec, forced)


def _f32(x):
    return x.detach().float().contiguous()


def _rows(m):
    """effective weight of a 1x1 holder module as [out][in] rows, and its bias: one weight-norm launch"""
    return _f32(W.normed_weight(m).reshape(m.bias.numel(), -1)), _f32(m.bias)


def _synth_weights(net, cond_on, fuse):
    """Every holder module's effective weight, computed once, as fp32 contiguous device tensors in the layouts of `viai_wn_layer` / `viai_wn_synth`.
    fuse: the fused stages (csrc/wavenet.hip, ABI 7) read gate_l from z_{l-1} and x_{l-1}(t) through extended rows
    [Wc^0 | Wc^1 | r Wc^2 | r Wc^2 Wo_prev] -- set-up arithmetic, once per synthesis call, in fp64 on the host: no library GEMM on the device path."""
    dev = net.first_conv.bias.device
    Cc = net.first_conv.bias.numel()
    r5 = math.sqrt(0.5)
    per = {k: [] for k in _LAYER_FIELDS}
    wo = bo = None                                                                    # fp64 host copies of the previous layer's out 1x1
    for f in net.conv_layers:
        lw = {}
        lw["w_conv"] = _f32(W.normed_weight(f.conv).permute(0, 2, 1).reshape(f.conv.bias.numel(), -1))     # linearised (conv.py:53-57)
        lw["b_conv"] = _f32(f.conv.bias)
        lw["w_c"], lw["b_c"] = _rows(f.conv1x1c) if (cond_on and f.conv1x1c is not None) else (None, None)
        lw["w_out"], lw["b_out"] = _rows(f.conv1x1_out)
        lw["w_skip"], lw["b_skip"] = _rows(f.conv1x1_skip)
        lw["w_stage"] = lw["b_stage"] = None
        if fuse:
            wlin, bias = lw["w_conv"].double().cpu(), lw["b_conv"].double().cpu()     # [Wc^0 | Wc^1 | Wc^2]
            if lw["b_c"] is not None:
                bias = bias + lw["b_c"].double().cpu()
            if wo is not None:
                wc2 = wlin[:, 2 * Cc:]
                wlin = torch.cat((wlin[:, :2 * Cc], r5 * wc2, r5 * (wc2 @ wo)), 1)
                bias = bias + r5 * (wc2 @ bo)
            lw["w_stage"], lw["b_stage"] = wlin.float().to(dev), bias.float().to(dev)
            wo, bo = lw["w_out"].double().cpu(), lw["b_out"].double().cpu()
        for k, v in lw.items():
            per[k].append(v)
    w_first, b_first = _rows(net.first_conv)                                          # [C] for the scalar input, [C][K] for the one-hot network
    w_first_t = None if net.scalar_input else w_first.t().contiguous()                # [K][C]: a class is one row
    return _Weights(*(per[k] for k in _LAYER_FIELDS), w_first, b_first, w_first_t,
                    *_rows(net.last_conv_layers[1]), *_rows(net.last_conv_layers[3]))


class _SynthState:
    """Every tensor the descriptor `desc` points to -- inputs, weights, rings, z / z2 / skips / step, out / logits / classes, g_add -- and the
    descriptor itself.  The kernels read and write these through raw pointers: the object must outlive the final stream synchronise of the run."""

    def __init__(self, net, inp, wts, fuse, softmax, quantize, log_scale_min, return_logits, return_classes):
        self.inp, self.wts = inp, wts
        cat, K, B, T = not net.scalar_input, net.out_channels, inp.B, inp.T
        dev = net.first_conv.bias.device
        Cc, G, S = net.first_conv.bias.numel(), net.conv_layers[0].conv.bias.numel(), net.conv_layers[0].conv1x1_skip.bias.numel()
        self.dilations = [f.conv.dilation[0] for f in net.conv_layers]
        self.rings = [torch.zeros(B, 2 * d + 1, Cc, device=dev) for d in self.dilations]
        # global conditioning adds conv1x1g(g) + bias to the gate pre-activation at every step (modules.py:195-199): computed once per layer by the
        # HIP 1x1 conv and handed to the step kernel as a per-stream constant
        self.g_add = [_f32(W.conv1d_apply(inp.g_vec.transpose(1, 2).reshape(B, 1, 1, -1).contiguous(), f.conv1x1g).reshape(B, G))
                      if (inp.g_vec is not None and f.conv1x1g is not None) else None for f in net.conv_layers]
        # categorical network: `out` is the head's scratch (hidden layer, logits), `logits` the (B, T, K) rows of the reference's `outputs`
        self.out = torch.zeros(B, S + K, device=dev) if cat else torch.zeros(B, T, device=dev)
        self.logits = torch.zeros(B, T, K, device=dev) if (return_logits or (cat and not return_classes)) else None
        self.classes = torch.zeros(B, T, dtype=torch.int32, device=dev) if cat else None
        self.z, self.z2 = torch.zeros(B, G // 2, device=dev), torch.zeros(B, G // 2, device=dev)
        self.skips = torch.zeros(B, S, device=dev)
        self.step = torch.zeros(1, dtype=torch.int32, device=dev)                     # time index, advanced on the device by each step
        self.layers = (_lib.WnLayer * len(self.dilations))()
        for i, (L, d) in enumerate(zip(self.layers, self.dilations)):
            for k in _LAYER_FIELDS:
                setattr(L, k, _ptr(getattr(wts, k)[i]))
            L.ring, L.dilation, L.ring_len, L.g_add = self.rings[i].data_ptr(), d, 2 * d + 1, _ptr(self.g_add[i])
        st = self.desc = _lib.WnSynth()
        st.B, st.C, st.G, st.S, st.cin, st.n_layers, st.out_ch, st.T = B, Cc, G, S, (inp.cond.size(2) if inp.cond is not None else 4), len(self.dilations), K, T
        st.n_test = inp.tin.size(1) if inp.tin is not None else (inp.tcls.size(1) if inp.tcls is not None else 0)
        st.log_scale_min = float(log_scale_min)
        st.layers = self.layers
        for k in _NET_FIELDS:
            setattr(st, k, _ptr(getattr(wts, k)))
        if cat:
            st.categorical, st.cat_softmax, st.cat_quantize, st.init_class = 1, int(bool(softmax)), int(bool(quantize)), 127 if K > 127 else 0
            st.test_classes, st.init_rows, st.classes = _ptr(inp.tcls), _ptr(inp.init_rows), self.classes.data_ptr()
        st.cond, st.test_inputs, st.u1, st.u2 = _ptr(inp.cond), _ptr(inp.tin), _ptr(inp.u1), inp.u2.data_ptr()
        st.out, st.z, st.z2, st.skips, st.step = self.out.data_ptr(), self.z.data_ptr(), self.z2.data_ptr(), self.skips.data_ptr(), self.step.data_ptr()
        st.yhat_dbg, st.fused = _ptr(self.logits), 1 if fuse else 0

    def result(self, return_logits, return_classes):
        if self.classes is not None:
            if return_classes:
                return self.classes.long()
            return self.logits.transpose(1, 2).contiguous()                           # (B, K, T) like the reference (wavenet.py:358-361)
        res = self.out.unsqueeze(1)                                                   # (B, 1, T) like the reference
        return (res, self.logits) if return_logits else res


def _synth_form(use_graph, fuse, pipe_env, pipe_ok, categorical_ok, cat, B, T, masked=False):
    """The launch form of a synthesis call.  "pipe": the pipelined form (csrc/wavenet_pipe.hip), one persistent launch, the stages work on
    different streams at the same time -- reference-size network with local conditioning only (pipe_ok: `viai_wn_pipe_ok`).  Everything else takes
    the chain of launches: "graph" (use_graph: one step with the time index on the device, captured once and replayed) or "chain" (the C side
    loops over the time steps).  pipe_env: VIAI_WN_PIPE != 0; categorical_ok: `viai_wn_categorical_ok`, looked at for the one-hot network only.
    masked: the call carries a mask of forced steps, which the chain forms take and the pipelined kernel does not."""
    pipe = (not use_graph) and fuse and pipe_env and pipe_ok and not masked
    if not pipe and B not in (1, 2, 4, 8):
        raise NotImplementedError("incremental_forward: the chain of launches takes 1, 2, 4 or 8 streams; any other count up to 32 needs the pipelined form "
                                  "(reference-size network, local conditioning only, no use_graph, VIAI_WN_PIPE != 0, a device with 256 compute units)")
    if cat and not categorical_ok:
        raise NotImplementedError("incremental_forward: the one-hot network needs out_channels <= 256 and a multiple of 4, channel counts that are multiples of 4")
    if pipe:
        return "pipe"
    return "graph" if use_graph and T > 2 else "chain"


def _timed_chunks(timing, T, chunk, launch, tqdm):
    """launch(t0, n) over [0, T) in chunks.  timing = {"warmup": W}: the first W steps are one untimed launch, the rest is bracketed by device
    synchronisations and reported as timing["ms"] / timing["steps"]."""
    w0 = min(int(timing.get("warmup", 0)), T) if timing is not None else 0
    if w0 > 0:
        launch(0, w0)
    if timing is not None:
        torch.cuda.synchronize()
        t_start = time.perf_counter()
    for t0 in tqdm(range(w0, T, chunk)):
        launch(t0, min(chunk, T - t0))
    if timing is not None:
        torch.cuda.synchronize()
        timing["ms"], timing["steps"] = (time.perf_counter() - t_start) * 1e3, T - w0


def _run_chain(lib, state, timing, tqdm):
    """default: the C side loops over the time steps and hands every kernel its time index by value"""
    ref, forced = Ct.byref(state.desc), state.inp.forced
    if forced is None:
        launch = lambda t0, n: _lib.check(lib.viai_wavenet_synth_run(ref, t0, n, _stream()), "viai_wavenet_synth_run")
    else:
        launch = lambda t0, n: _lib.check(lib.viai_wavenet_synth_run_forced(ref, forced.data_ptr(), t0, n, _stream()), "viai_wavenet_synth_run_forced")
    _timed_chunks(timing, state.inp.T, 64, launch, tqdm)


def _run_graph(lib, state, timing, tqdm):
    """device-side time index: one step captured into a HIP graph and replayed (every kernel starts with a load of the index)"""
    ref, forced = Ct.byref(state.desc), state.inp.forced
    if forced is None:
        step = lambda: _lib.check(lib.viai_wavenet_synth_step(ref, _stream()), "viai_wavenet_synth_step")
    else:
        step = lambda: _lib.check(lib.viai_wavenet_synth_step_forced(ref, forced.data_ptr(), _stream()), "viai_wavenet_synth_step_forced")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                                        # step 0 (warm-up)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()                                                                        # captured: step 1
    for _ in tqdm(range(state.inp.T - 1)):
        graph.replay()


def _run_pipe(lib, state, timing, tqdm):
    ref, w, B, dev = Ct.byref(state.desc), state.wts, state.inp.B, state.out.device
    imgs = _pipe_images(w.w_stage, w.b_stage, w.w_c, w.w_out, w.b_out, w.w_skip, w.b_skip, w.w_l1, w.b_l1, w.w_l2, w.b_l2, dev)
    for k, im in enumerate((imgs[0], imgs[2], imgs[3], imgs[4], imgs[5], imgs[1])):
        assert im.numel() == lib.viai_wn_pipe_image_floats(k), (k, im.numel(), lib.viai_wn_pipe_image_floats(k))
    dil = (Ct.c_int * len(state.dilations))(*state.dilations)
    tok = torch.zeros(lib.viai_wn_pipe_token_granules(B, dil), dtype=torch.int64, device=dev)
    err = torch.zeros(4, dtype=torch.int32, device=dev)

    def launch(t0, n):
        _lib.check(lib.viai_wn_pipe_run(ref, *(im.data_ptr() for im in imgs), tok.data_ptr(), err.data_ptr(), t0, n, _stream()), "viai_wn_pipe_run")
    _timed_chunks(timing, state.inp.T, 1024, launch, tqdm)
    if timing is not None:
        timing["form"] = "pipe"
    e = err.tolist()
    if e[0] != 0:
        raise _lib.ViaiLibraryError("viai_wn_pipe_run failed on the device: %s at stage %d, stream %d, t = %d (the pipelined form needs all of its 249 blocks "
                                    "resident at once, i.e. the whole chip to itself; VIAI_WN_PIPE=0 selects the chain of launches)"
                                    % ("a wait timed out" if e[0] == 1 else "a past tap was missing", e[1], e[2], e[3]))


_RUNNERS = {"pipe": _run_pipe, "graph": _run_graph, "chain": _run_chain}


def incremental_forward(net, initial_input, c, g, T, test_inputs, tqdm, softmax, quantize, log_scale_min, uniforms, use_graph, return_logits,
                        timing, return_classes, input_form, forced=None, c_upsampled=False):
    """`WaveNet.incremental_forward` (documented there)."""
    inp = _resolve_inputs(net, initial_input, c, g, T, test_inputs, softmax, quantize, uniforms, return_logits, return_classes, input_form, forced,
                          c_upsampled)
    lib = _lib.load()
    f0 = net.conv_layers[0]
    fuse = (os.environ.get("VIAI_WN_FUSED", "1") != "0" and f0.conv1x1_skip.bias.numel() <= 256 and net.out_channels <= 256
            and f0.conv.bias.numel() // 2 <= 256)
    state = _SynthState(net, inp, _synth_weights(net, inp.cond is not None, fuse), fuse, softmax, quantize, log_scale_min, return_logits, return_classes)
    ref = Ct.byref(state.desc)
    form = _synth_form(use_graph, fuse, os.environ.get("VIAI_WN_PIPE", "1") != "0", bool(lib.viai_wn_pipe_ok(ref)),
                       bool(lib.viai_wn_categorical_ok(ref)), not net.scalar_input, inp.B, inp.T, inp.forced is not None)
    _RUNNERS[form](lib, state, timing, tqdm)
    torch.cuda.current_stream().synchronize()
    return state.result(return_logits, return_classes)


def _pipe_images(w_stage, b_stage, w_c, w_out, b_out, w_skip, b_skip, w_l1, b_l1, w_l2, b_l2, dev):
    """Weight images of the pipelined synthesis kernel (csrc/wavenet_pipe.hip; layouts in include/viai_hip.h, viai_wn_pipe_image_floats).
    Inputs: per layer the fused gate rows `w_stage[l]` [G][3C (+H for l > 0)] / `b_stage[l]` [G] of the chain form, the conditioning rows `w_c[l]`
    [G][cin], and the out / skip 1x1s; the head's two 1x1s.  Compute unit j of layer l owns gate pairs h in [26 j, 26 j + 26), residual rows
    [52 j, 52 j + 52) and skip rows [26 j, 26 j + 26) -- row SLOTS beyond a range are zero rows.  Pure re-arrangement: no arithmetic on the weights."""
    NL, NCU, NW, GW, BW, C, H, S = 24, 10, 8, 7, 10, 512, 256, 256
    G = 2 * H
    j = torch.arange(NCU).view(NCU, 1)
    r = torch.arange(NW * GW).view(1, -1)
    hh = 26 * j + torch.where(r < 26, r, r - 26)
    grow = torch.where((r < 52) & (hh < H), hh + torch.where(r < 26, 0, H), torch.full_like(hh, G)).to(dev)          # [10][56] -> gate row, G = the zero row
    q = torch.arange(NW * BW).view(1, -1)
    xrow = 52 * j + q
    srow = 26 * j + (q - 52)
    # B slots: < 52 residual row, 52 .. 77 skip row (offset C in the stacked [Wo; Ws] matrix), C + S = the zero row
    brow = torch.where((q < 52) & (xrow < C), xrow, torch.where((q >= 52) & (q < 78) & (srow < S), C + srow, torch.full_like(xrow, C + S))).to(dev)
    wreg, wcond, wlds, bias = [], [], [], []
    z1 = lambda n: torch.zeros(1, n, device=dev)
    for l in range(NL):
        ws = w_stage[l]
        if ws.size(1) == 3 * C:
            ws = torch.cat((ws, torch.zeros(G, H, device=dev)), 1)                      # layer 0: no z columns
        W = torch.cat((ws, z1(3 * C + H)), 0)[grow]                                     # [10][56][1792]
        # register image: wave = 128 past-tap / 64 current-tap columns of all 52 rows; lane (g, cg) = (lane / 16, lane % 16) holds rows 13 g + i (i < 13):
        # register 8 i + 4 m + e = past-tap column 128 wave + 64 m + 4 cg + e, register 104 + 4 i + e = current-tap column 64 wave + 4 cg + e
        pre = W[:, :52, :2 * C].reshape(NCU, 4, 13, NW, 2, 16, 4).permute(0, 3, 2, 4, 6, 1, 5).reshape(NCU, NW, 104, 64)
        cur = W[:, :52, 2 * C:3 * C].reshape(NCU, 4, 13, NW, 16, 4).permute(0, 3, 2, 5, 1, 4).reshape(NCU, NW, 52, 64)
        wreg.append(torch.cat((pre, cur), 2))                                           # 104 + 52 registers
        wc = torch.cat((w_c[l], z1(w_c[l].size(1))), 0)[grow]                           # [10][56][80]
        wcond.append(torch.cat((wc, torch.zeros(NCU, 8, wc.size(2), device=dev)), 1))   # 64 row slots
        bg = torch.cat((b_stage[l], torch.zeros(1, device=dev)))[grow]                  # [10][56]
        if l == 0:
            wB, bB = torch.zeros(NCU, NW * BW, H, device=dev), torch.zeros(NCU, NW * BW, device=dev)
        else:
            wB = torch.cat((w_out[l - 1], w_skip[l - 1], z1(H)), 0)[brow]               # [10][80][256]
            bB = torch.cat((b_out[l - 1], b_skip[l - 1], torch.zeros(1, device=dev)))[brow]
        rows = torch.cat((W[:, :52, 3 * C:], wB[:, :78]), 1)                            # LDS rows: 52 gate rows (z columns), 78 out / skip rows
        wlds.append(torch.nn.functional.pad(rows, (0, 4)))                              # rows padded to 260 floats (lane = row reads without bank conflicts)
        bias.append(torch.cat((bg, bB), 1))
    head_w = torch.cat((w_skip[NL - 1], w_l1, w_l2, torch.zeros(32 - w_l2.size(0), S, device=dev)), 0)
    head_b = torch.cat((b_skip[NL - 1], b_l1, b_l2, torch.zeros(32 - b_l2.numel(), device=dev)))
    c = lambda ts: torch.stack(ts).float().contiguous()
    return c(wreg), c(wcond), c(wlds), c(bias), head_w.float().contiguous(), head_b.float().contiguous()
