"""GPU: every launch form and branch of a WaveNet synthesis time step (csrc/wavenet.hip from wn_first_kernel on, csrc/wavenet_pipe.hip) against the
fp64 ring oracle (oracle.incremental_forward_ring(dtype=torch.float64)) on the same fp32 weights and inputs, ROW BY ROW: a row is the logits of one stream at
one time step, its error max_k |got - truth| / max(max_k |truth|, the run's median row maximum), and the assertion is on the worst row of a run.

Bound: MARGIN = 4 x the worst row of the SAME ring algorithm evaluated by torch in fp32 on the CPU (the oracle's default dtype), same inputs, same measure
(the rule of tests/test_wavenet_train_kernels_gpu.py; 4 allows another, equally valid fp32 summation order).  Every figure is printed beside its yardstick
before the assertion; DESIGN.md section 11.2 holds the table measured on the MI355X.

Networks (tests/wavenet_synth_common.py NETS; weight-normalised like the reference, conditioning at the sample rate), T = 24 (140 for `deep`): at least
twice the longest ring plus 5.  Runs (RUNS): B in 1, 2, 4, 8 occurs in every form family (chain unfused, chain fused, graph), no full product.

Branch table (kernels per time step from wn_step_impl / wn_step_fused_impl / wn_cat_head; tests/test_wavenet_synth_forms_cpu.py derives the same on the host
from the shapes and asserts that every switch is taken both ways):

  network     C / G (H) / S / cin / layers  fused form (wn_fused_ok)      head, unfused             head, fused                          B: unfused / fused / graph
  floor       4 / 8 (4) / 4 / 4 / 2         yes                           wn_head_kernel            wn_head_rows x 2 + wn_head_sample    1 / 8 / 4   (+ B1 without c)
  ragged      100 / 136 (68) / 36 / 20 / 3  yes                           wn_head_kernel            rows + sample (S <= H)               2 / 4 / 1, graph unfused 8; masks 4 / 2 / 8
  rows-head   32 / 128 (64) / 32 / 80 / 4   yes                           wn_head_kernel            rows + sample                        4 / 1 / 8
  fused-head  32 / 32 (16) / 32 / 80 / 4    yes                           wn_head_kernel            wn_head_fused_kernel (S > H)         8 / 2 / 4   (+ fused B8 without c)
  wide-skip   64 / 64 (32) / 260 / 80 / 2   refused: S > 256              wn_head_generic_kernel    --                                   2 / 1 / 8   (all three run unfused)
  wide-gate   16 / 520 (260) / 16 / 4 / 2   refused: G / 2 > 256          wn_head_kernel            --                                   4 / 8 / 1   (all three run unfused)
  deep        8 / 16 (8) / 8 / 4 / 6        yes                           wn_head_kernel            rows + sample                        1 / 2 / 4   dilations 1 .. 32
  global      12 / 24 (12) / 12 / 4 / 2     yes; g_add in every gate      wn_head_kernel            rows + sample                        8 / 1 / 2 with c, 2 / 4 / 8 without
  onehot K    12 / 24 (12) / 12 / 4 / 2     yes                           wn_cat_rows x 2 + wn_cat_sample (both forms; fused: wn_head_rows first)
              K = 256: 1 / 8 dense / 2;  68: 2 dense / 4 / 1 dense, masks 8 / 2 (mixed class and dense streams);  12: 4 / 2 dense / 8;  4: 8 dense / 1 / 4
  single      12 / 24 (12) / 12 / 4 / 1     yes; n == 1: first skip = last  wn_head_kernel          rows + sample (first_skip = 1)       2 / 8 / 1;  K = 12 one-hot: 4 / 1 dense / 2
  unfused step: wn_first_kernel (one-hot: wn_cat_first_kernel, class or dense form), then wn_gate_kernel<B> + wn_out_kernel<B> per layer, then the head.
  fused step:   [wn_tick_kernel under a graph] [wn_cat_first_kernel<B>(dense_only) for dense one-hot rows] wn_stage_kernel<B> per layer (stage 0 forms the
                first conv, stage l > 0 also layer l - 1's out / skip rows; first_skip at l == 1), then the head (the last layer's skip rows move into it).
  time index:   chain forms by value (viai_wavenet_synth_run[_forced]), graph form from device memory (viai_wavenet_synth_step[_forced] replayed).
  pipelined:    reference-size network only (build_cfg(WNConfigFull)), B = 1 and 3 (3 streams are taken by this form alone), T = 140, one launch and two.
The out_ch > 256 side of wn_fused_ok / the head switch is not reached: the one-hot network stops at 256 classes (viai_wn_categorical_ok) and the mixture head
has 30 outputs.

Sampler edges: a network whose last 1x1 has weight_g = 0 emits its bias as logits at every step exactly, which hands chosen rows to the sampler tail of every
head kernel (wavenet_synth_common.mol_edge_cases / cat_edge_uniforms); viai_mol_sample is also called directly.
"""
import pytest
import torch

import wavenet_synth_common as S
from oracle import viai_oracle as O
from oracle import wavenet_oracle as W

pytestmark = pytest.mark.gpu

_ORACLE = {}


def make_net(name, sd=None):
    from viai_amd.wavenet import WaveNet
    cfg, sd0 = S.state(name)
    sd = sd0 if sd is None else sd
    net = WaveNet(out_channels=cfg.out_channels, layers=cfg.layers, stacks=cfg.stacks, residual_channels=cfg.residual_channels,
                  gate_channels=cfg.gate_channels, skip_out_channels=cfg.skip_out_channels, kernel_size=cfg.kernel_size, dropout=0.0,
                  cin_channels=cfg.cin_channels, gin_channels=cfg.gin_channels, n_speakers=cfg.n_speakers, weight_normalization=True,
                  upsample_conditional_features=True, upsample_scales=list(cfg.upsample_scales), freq_axis_kernel_size=cfg.freq_axis_kernel_size,
                  scalar_input=cfg.scalar_input)
    assert list(net.state_dict().keys()) == list(sd.keys())
    net.load_state_dict(sd)
    return net.cuda().eval()


@pytest.fixture(scope="module")
def nets():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = (make_net(name), S.state(name)[1])
        return cache[name]
    return get


def set_form(monkeypatch, form):
    monkeypatch.setenv("VIAI_WN_FUSED", "0" if form.endswith("unfused") else "1")
    return form.startswith("graph")


def cu(t):
    return None if t is None else t.cuda()


def gpu_scalar(net, d, x, graph, mask=None, lsm=S.LOG_SCALE_MIN):
    """(out (B, 1, T), logits (B, T, 30)) of the mixture network"""
    out, lg = net.incremental_forward(None, c=cu(d["c"]), g=cu(d["g"]), T=d["T"], test_inputs=cu(x), log_scale_min=lsm, uniforms=(d["u1"], d["u2"]),
                                      use_graph=graph, return_logits=True, forced=cu(mask), c_upsampled=True)
    return out.cpu(), lg.cpu()


def gpu_cat(net, d, x, graph, softmax, quantize=False, mask=None, dense=False, classes=False):
    """(B, T, K) rows of the one-hot network (logits / probabilities / one-hot rows), or the (B, T) classes"""
    y = net.incremental_forward(None, c=cu(d["c"]), g=cu(d["g"]), T=d["T"], test_inputs=cu(x), softmax=softmax, quantize=quantize, uniforms=d["u2"],
                                use_graph=graph, input_form="dense" if dense else "auto", forced=cu(mask), c_upsampled=True, return_classes=classes)
    return y.cpu() if classes else y.transpose(1, 2).contiguous().cpu()


def truth_and_yard(r, sd, d, x, key):
    if key not in _ORACLE:
        _ORACLE[key] = (S.oracle_logits(r.net, sd, d, x, torch.float64), S.oracle_logits(r.net, sd, d, x, None))
    return _ORACLE[key]


# ================================================================================================================== teacher-forced, every run
@pytest.mark.parametrize("r", S.RUNS, ids=[S.run_id(r) for r in S.RUNS])
def test_teacher_forced_logits_row_by_row(r, nets, monkeypatch):
    net, sd = nets(r.net)
    graph = set_form(monkeypatch, r.form)
    d = S.inputs(r)
    scalar, K = S.NETS[r.net][7], S.NETS[r.net][6]
    what = S.run_id(r)
    if scalar:
        out, lg = gpu_scalar(net, d, d["x"], graph, d["mask"])
        x = d["x"] if d["mask"] is None else S.effective_inputs(d, out, True, K)     # under a mask: what every step actually consumed
        truth, yard = truth_and_yard(r, sd, d, x, what if d["mask"] is not None else (r.net, r.B, r.opts))
        S.check_rows(lg, truth, yard, what + " logits")
        return
    if d["mask"] is not None:
        # forced streams take the class form, the others are fed the previous probabilities (dense rows): no compounding, the oracle is teacher-forced
        # on what the GPU fed back
        p = gpu_cat(net, d, d["x"], graph, softmax=True, mask=d["mask"])
        x = S.effective_inputs(d, p.transpose(1, 2), False, K)
        truth, yard = truth_and_yard(r, sd, d, x, what)
        S.check_rows(p, torch.softmax(truth, -1), torch.softmax(yard, -1), what + " probabilities")
        return
    truth, yard = truth_and_yard(r, sd, d, d["x"], (r.net, r.B, ()))
    dense = "dense" in r.opts
    lg = gpu_cat(net, d, d["x"], graph, softmax=False, dense=dense)
    S.check_rows(lg, truth, yard, what + " logits")
    p = gpu_cat(net, d, d["x"], graph, softmax=True, dense=dense)
    S.check_rows(p, torch.softmax(truth, -1), torch.softmax(yard, -1), what + " probabilities")
    assert float((p.sum(-1) - 1).abs().max()) < 1e-5


# ========================================================================================================== free-running without compounding
@pytest.mark.parametrize("form", ["unfused", "fused", "graph"])
def test_free_running_scalar_hand_off_step_by_step(form, nets, monkeypatch):
    """three forced samples, then the GPU runs free with injected uniforms; the fp64 oracle is then teacher-forced on the GPU's OWN outputs shifted by one,
    so every row checks one sampler-to-stage-0 hand-off and nothing compounds"""
    r = S.Run("ragged", form, 4, ())
    net, sd = nets(r.net)
    graph = set_form(monkeypatch, form)
    d = S.inputs(r)
    d["x"], d["n_prefix"] = d["x"][:, :, :3].contiguous(), 3
    out, lg = gpu_scalar(net, d, d["x"], graph)
    assert float(out.abs().max()) <= 1.0 and out[:, 0, 3:].unique().numel() > d["T"]
    x = S.effective_inputs(d, out, True, 30)
    S.check_rows(lg, S.oracle_logits(r.net, sd, d, x, torch.float64), S.oracle_logits(r.net, sd, d, x, None), "ragged-%s-B4 free-running logits" % form)


@pytest.mark.parametrize("form", ["unfused", "fused", "graph"])
def test_free_running_one_hot_hand_off_step_by_step(form, nets, monkeypatch):
    """one-hot network, three forced classes, then (a) softmax=True / quantize=False: the probabilities are fed back as dense rows, the oracle is fed the GPU's
    rows; (b) quantize=True: the drawn class is fed back, the oracle is fed the GPU's classes -- the GPU returns no logits in that mode, so the check is the
    draw itself: at every step the GPU's class is the fp64 inverse-cdf class of the oracle's probabilities, unless u lies within 4 x the fp32 restatement's
    worst cdf error of an fp64 edge (the yardstick rule on the cdf; such a step decides nothing, and at most one in ten may be of that kind)"""
    r = S.Run("onehot68", form, 4, ())
    net, sd = nets(r.net)
    graph = set_form(monkeypatch, form)
    d = S.inputs(r)
    K, T = 68, d["T"]
    d["x"], d["n_prefix"] = d["x"][:, :, :3].contiguous(), 3
    p = gpu_cat(net, d, d["x"], graph, softmax=True)
    x = S.effective_inputs(d, p.transpose(1, 2), False, K)
    t64, t32 = S.oracle_logits(r.net, sd, d, x, torch.float64), S.oracle_logits(r.net, sd, d, x, None)
    S.check_rows(p, torch.softmax(t64, -1), torch.softmax(t32, -1), "onehot68-%s-B4 free-running probabilities (dense feedback)" % form)
    cls = gpu_cat(net, d, d["x"], graph, softmax=True, quantize=True, classes=True)
    hot = gpu_cat(net, d, d["x"], graph, softmax=True, quantize=True)
    assert torch.equal(hot.argmax(-1), cls) and torch.equal(hot.sum(-1), torch.ones(4, T)) and bool(((hot == 0) | (hot == 1)).all())
    xc = S.effective_inputs(d, torch.nn.functional.one_hot(cls, K).float().transpose(1, 2), False, K)
    c64, c32 = (torch.cumsum(torch.softmax(S.oracle_logits(r.net, sd, d, xc, dt).double(), -1), -1) for dt in (torch.float64, None))
    tol = S.MARGIN * float((c32 - c64).abs().max())
    u = d["u2"].double()
    want = (c64 <= u.unsqueeze(-1)).sum(-1).clamp(max=K - 1)
    decisive = (c64[..., :K - 1] - u.unsqueeze(-1)).abs().amin(-1) > tol
    print("onehot68-%s-B4 sampled: %d of %d steps decisive at cdf tolerance %.3e, classes drawn %d" % (form, int(decisive.sum()), decisive.numel(), tol, cls.unique().numel()))
    assert int(decisive.sum()) >= 0.9 * decisive.numel() and cls.unique().numel() > 8
    bad = (decisive & (cls != want)).nonzero()
    assert bad.numel() == 0, "stream %d, step %d: drew %d, fp64 inverse cdf %d" % (int(bad[0, 0]), int(bad[0, 1]), int(cls[tuple(bad[0])]), int(want[tuple(bad[0])]))


# ======================================================================================================================== the pipelined form
@pytest.fixture(scope="module")
def full_net():
    """the 24.7 M-parameter network, built once per module"""
    from test_wavenet_gpu import build_cfg
    return build_cfg(W.WNConfigFull, "WN.").eval(), W.wavenet_state(W.WNConfigFull, "WN.")


PIPE_T = 140


def pipe_inputs(B):
    cfg = W.WNConfigFull
    tag = "wnsf.pipe.%d." % B
    return {"T": PIPE_T, "c": O.cf_uniform(tag + "c", (B, cfg.cin_channels, PIPE_T), 0, 1), "g": None, "x": O.cf_uniform(tag + "x", (B, 1, PIPE_T), -1, 1),
            "u1": O.cf_uniform(tag + "u1", (B, PIPE_T, 10), 1e-5, 1 - 1e-5), "u2": O.cf_uniform(tag + "u2", (B, PIPE_T), 1e-5, 1 - 1e-5)}


def pipe_run(net, d, timing, lsm=S.LOG_SCALE_MIN):
    out, lg = net.incremental_forward(None, c=d["c"].cuda(), T=d["T"], test_inputs=d["x"].cuda(), log_scale_min=lsm, uniforms=(d["u1"], d["u2"]),
                                      return_logits=True, c_upsampled=True, timing=timing)
    assert timing.get("form") == "pipe"
    return out.cpu(), lg.cpu()


@pytest.mark.parametrize("B", [1, 3])
def test_pipelined_form_logits_row_by_row(B, full_net, monkeypatch):
    """reference size, T = 140 (the 65-slot rings wrap twice), teacher-forced; B = 3 also as two launches [0, 67) and [67, 140): bitwise the single launch.
    (The fp64 oracle at this size: 1.6 s for 4 streams x 140 steps on 8 CPU threads.)"""
    monkeypatch.setenv("VIAI_WN_FUSED", "1")
    monkeypatch.setenv("VIAI_WN_PIPE", "1")
    net, sd = full_net
    d = pipe_inputs(B)
    out, lg = pipe_run(net, d, {"warmup": 0})
    cfg = W.WNConfigFull
    run = lambda dt: W.incremental_forward_ring(sd, d["c"], PIPE_T, d["u1"], d["u2"], cfg, test_inputs=d["x"], return_logits=True, dtype=dt)[1].transpose(1, 2)
    S.check_rows(lg, run(torch.float64), run(None), "reference size, pipelined, B%d logits" % B)
    if B == 3:
        from viai_amd import _lib
        lib, ran = _lib.load(), []
        real = lib.viai_wn_pipe_run
        monkeypatch.setattr(lib, "viai_wn_pipe_run", lambda *a: (ran.append(a[-3:-1]), real(*a))[1], raising=False)
        out2, lg2 = pipe_run(net, d, {"warmup": 67})
        assert ran == [(0, 67), (67, PIPE_T - 67)]
        assert torch.equal(lg2, lg) and torch.equal(out2, out)


# ================================================================================================= sampler edges through every copy: mixture
MOL_HEADS = [("floor", "unfused", "wn_head_kernel"), ("wide-skip", "unfused", "wn_head_generic_kernel"), ("fused-head", "fused", "wn_head_fused_kernel"),
             ("rows-head", "fused", "wn_head_sample_kernel"), ("fused-head", "graph", "wn_head_fused_kernel, time index on the device")]


def check_mol_case(name, got, lg, row, lsm, u1, u2, clipped, what):
    v64, comp, score = S.mol_truth(row, lsm, u1, u2, torch.float64)
    v32 = S.mol_truth(row, lsm, u1, u2, torch.float32)[0]
    top2 = score.topk(2, -1).values
    assert float((top2[..., 0] - top2[..., 1]).min()) >= 1e-3, what                   # no near tie: the fp64 winner is the winner
    if lg is not None:
        assert torch.equal(lg, row.reshape(1, 1, -1).expand_as(lg)), what + ": the logits are not the bias row"
    got = got.double().reshape(v64.shape)
    err, yard = float((got - v64).abs().max()), float((v32.double() - v64).abs().max())
    print("%-64s %-12s max |x - fp64| %.3e   fp32 torch %.3e" % (what, name, err, yard))
    if clipped:
        want = torch.where(u2 < 0.5, -1.0, 1.0).double()
        assert torch.equal(v64, want) and torch.equal(got, want), what + ": a clipped value is exactly -1 or 1"
    else:
        bad = (S.component_of(got) != comp).nonzero()
        assert bad.numel() == 0, "%s %s: stream %d step %d took component %d, fp64 %d" % (what, name, *bad[0].tolist(), int(S.component_of(got)[tuple(bad[0])]), int(comp[tuple(bad[0])]))
        assert err <= S.MARGIN * yard, (what, name, err, yard)


@pytest.mark.parametrize("netname,form,kernel", MOL_HEADS, ids=[m[2].split(",")[0] + "-" + m[1] for m in MOL_HEADS])
def test_mixture_sampler_edges_through_each_head_kernel(netname, form, kernel, monkeypatch):
    graph = set_form(monkeypatch, form)
    r = S.Run(netname, form, 2, ())
    assert S.switches(r)[1][-1] == kernel.split(",")[0]
    d = S.inputs(r)
    cfg, sd = S.state(netname)
    for name, (row, lsm, u1, u2, clipped) in S.mol_edge_cases(B=2, T=d["T"]).items():
        sd2 = dict(sd)
        sd2["last_conv_layers.3.weight_g"] = torch.zeros_like(sd["last_conv_layers.3.weight_g"])
        sd2["last_conv_layers.3.bias"] = row.clone()
        net = make_net(netname, sd2)
        d["u1"], d["u2"] = u1, u2
        out, lg = gpu_scalar(net, d, d["x"], graph, lsm=lsm)
        check_mol_case(name, out[:, 0], lg, row, lsm, u1, u2, clipped, kernel)


def test_mixture_sampler_edges_through_the_pipelined_tail(full_net, monkeypatch):
    monkeypatch.setenv("VIAI_WN_FUSED", "1")
    monkeypatch.setenv("VIAI_WN_PIPE", "1")
    net, _ = full_net
    last = net.last_conv_layers[3]
    keep = (last.weight_g.data.clone(), last.bias.data.clone())
    d = pipe_inputs(3)
    d["T"] = T = S.MOL_T
    d["c"], d["x"] = d["c"][:, :, :T].contiguous(), d["x"][:, :, :T].contiguous()
    try:
        last.weight_g.data.zero_()
        for name, (row, lsm, u1, u2, clipped) in S.mol_edge_cases(B=3, T=T).items():
            last.bias.data.copy_(row)
            d["u1"], d["u2"] = u1, u2
            out, lg = pipe_run(net, d, {"warmup": 0}, lsm)
            check_mol_case(name, out[:, 0], lg, row, lsm, u1, u2, clipped, "pipelined tail")
    finally:
        last.weight_g.data.copy_(keep[0])
        last.bias.data.copy_(keep[1])


@pytest.mark.parametrize("pitch,rows", [(32, 1), (40, 1), (32, 257), (40, 257), (32, 8192 * 256 + 1)])
def test_mol_sample_kernel_edges_direct(pitch, rows):
    """viai_mol_sample at the C ABI: pitch 32 / 40, one row, a ragged second block, and one row past the grid cap of ew_blocks (8192 blocks of 256: the
    grid-stride loop takes a second trip for exactly one row).  The rows are the edge cases block by block, tiled with a period of 6 x 41 = 246 rows, which
    divides neither 256 nor the grid's stride, so a row read at the wrong index shows."""
    from viai_amd.wavenet import mol_sample
    per = 41
    cases = S.mol_edge_cases(B=1, T=per)
    for lsm_name in ("clamp-below", "clamp-at", "clamp-above"):
        lsm = cases[lsm_name][1]
        base_y, base_u1, base_u2, base_v64, base_v32, base_comp, base_clip = [], [], [], [], [], [], []
        for name, (row, _, u1, u2, clipped) in cases.items():
            v64, comp, score = S.mol_truth(row, lsm, u1, u2, torch.float64)
            top2 = score.topk(2, -1).values
            assert float((top2[..., 0] - top2[..., 1]).min()) >= 1e-3
            base_y.append(torch.nn.functional.pad(row, (0, pitch - 30)).reshape(1, pitch).expand(per, pitch))
            base_u1.append(u1[0]); base_u2.append(u2[0]); base_v64.append(v64[0]); base_v32.append(S.mol_truth(row, lsm, u1, u2, torch.float32)[0][0].double())
            base_comp.append(comp[0]); base_clip.append(torch.full((per,), clipped))
        cat = lambda ts: torch.cat(ts, 0)
        reps = -(-rows // (6 * per))
        tile = lambda t: t.repeat((reps,) + (1,) * (t.dim() - 1))[:rows].contiguous()
        y, u1, u2 = tile(cat(base_y)), tile(cat(base_u1)), tile(cat(base_u2))
        v64, v32, comp, clip = tile(cat(base_v64)), tile(cat(base_v32)), tile(cat(base_comp)), tile(cat(base_clip))
        got = mol_sample(y.cuda(), u1.cuda(), u2.cuda(), lsm).double().cpu()
        err, yard = float((got - v64).abs().max()), float((v32 - v64).abs().max())
        print("viai_mol_sample pitch %d rows %d log_scale_min %-9.6g max |x - fp64| %.3e   fp32 torch %.3e" % (pitch, rows, lsm, err, yard))
        assert torch.equal(got[clip], v64[clip]) and bool((got[clip].abs() == 1).all())
        bad = ((S.component_of(got) != comp) & ~clip).nonzero()
        assert bad.numel() == 0, "row %d took another component" % int(bad[0])
        assert err <= S.MARGIN * yard, (err, yard)
        if rows > 1000:
            break                                                                     # the large count once


# ============================================================================================= sampler edges through wn_cat_sample_kernel
@pytest.mark.parametrize("form", ["unfused", "fused", "graph"])
@pytest.mark.parametrize("K", S.CAT_KS)
def test_categorical_draw_edges(K, form, monkeypatch):
    """softmax=True, quantize=True on a network that emits a chosen logits row at every step; u per step at 0, 3e-5 either side of class edges and
    1 - 1e-7 (wavenet_synth_common.cat_edge_uniforms; none within 1e-5 of an fp64 edge -- asserted): the class is the fp64 inverse-cdf class exactly, the
    one-hot row is 1 there and 0 elsewhere, `classes` holds the same index.  Stream b of B = 2 takes the draws in reverse order."""
    graph = set_form(monkeypatch, form)
    name = {256: "onehot256", 68: "onehot68", 12: "onehot12", 4: "onehot4"}[K]
    cfg, sd = S.state(name)
    for kind, row in S.cat_rows(K).items():
        u, want, dropped = S.cat_edge_uniforms(row)
        assert dropped == 0
        T = u.numel()
        r = S.Run(name, form, 2, ())
        d = S.inputs(r, T=T)
        d["u2"] = torch.stack((u, u.flip(0)))
        want2 = torch.stack((want, want.flip(0)))
        sd2 = dict(sd)
        sd2["last_conv_layers.3.weight_g"] = torch.zeros_like(sd["last_conv_layers.3.weight_g"])
        sd2["last_conv_layers.3.bias"] = row.clone()
        net = make_net(name, sd2)
        lg = gpu_cat(net, d, d["x"], graph, softmax=False)
        assert torch.equal(lg, row.reshape(1, 1, K).expand(2, T, K))
        cls = gpu_cat(net, d, d["x"], graph, softmax=True, quantize=True, classes=True)
        hot = gpu_cat(net, d, d["x"], graph, softmax=True, quantize=True)
        bad = (cls != want2).nonzero()
        assert bad.numel() == 0, "K %d %s %s: stream %d u %.9g: drew %d, fp64 inverse cdf %d" % (
            K, kind, form, int(bad[0, 0]), float(d["u2"][tuple(bad[0])]), int(cls[tuple(bad[0])]), int(want2[tuple(bad[0])]))
        assert torch.equal(hot, torch.nn.functional.one_hot(want2, K).float())
