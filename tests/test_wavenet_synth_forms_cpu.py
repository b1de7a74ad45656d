"""No GPU: what tests/test_wavenet_synth_forms_gpu.py rests on.
  1. oracle.incremental_forward_ring(dtype=): the fp32 default still reproduces the reference's goldens (mixture network: tests/golden/wavenet.npz; one-hot
     network, new in the ring form: tests/golden/wavenet_onehot_synth.npz -- probabilities, logits and every drawn class), and fp64 agrees with it to fp32 rounding.
  2. The per-row measure is worth having: three localized defects in the fp32 restatement each exceed the per-row bound on the `ragged` network; the
     Frobenius-relative figure of the older tests is printed beside each (several times smaller: it averages over the rows the defect does not reach).
  3. The list of runs takes every switch of a synthesis step both ways (derived on the host from the shapes; nothing is launched).
  4. The categorical sampler-edge draws are constructed so that none lies within 1e-5 of an fp64 class edge, for all four K."""
import os

import numpy as np
import pytest
import torch

import wavenet_synth_common as S
from oracle import viai_oracle as O
from oracle import wavenet_oracle as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def relerr(a, b):
    a, b = torch.as_tensor(a).double().reshape(-1), torch.as_tensor(b).double().reshape(-1)
    return float((a - b).norm() / b.norm())


# ---------------------------------------------------------------------------------------------------------------------------- 1. the oracle
def test_ring_oracle_default_dtype_reproduces_the_goldens_and_fp64_agrees_to_fp32_rounding(golden_dir):
    g2 = np.load(golden_dir + "/wavenet.npz")
    cfg, sd = W.WNConfig, W.wavenet_state(W.WNConfig)
    cg = O.cf_uniform("wn.cg", (2, cfg.cin_channels, 2), 0, 1)
    v1, v2 = O.cf_uniform("wn.v1", (2, 32, 10), 1e-5, 1 - 1e-5), O.cf_uniform("wn.v2", (2, 32), 1e-5, 1 - 1e-5)
    tin = O.cf_uniform("wn.tin", (2, 1, 4), -1, 1)
    gen = W.incremental_forward_ring(sd, cg, 32, v1, v2, cfg, test_inputs=tin)
    assert gen.dtype == torch.float32 and relerr(gen, g2["gen"]) < 1e-4
    # teacher-forced over the whole length (nothing compounds): fp64 and fp32 logits agree row by row to fp32 rounding
    x = O.cf_uniform("wn.tf", (2, 1, 32), -1, 1)
    o32, l32 = W.incremental_forward_ring(sd, cg, 32, v1, v2, cfg, test_inputs=x, return_logits=True)
    o64, l64 = W.incremental_forward_ring(sd, cg, 32, v1, v2, cfg, test_inputs=x, return_logits=True, dtype=torch.float64)
    assert (o32.dtype, l32.dtype, o64.dtype, l64.dtype) == (torch.float32, torch.float32, torch.float64, torch.float64)
    e = S.worst_row(l32.transpose(1, 2), l64.transpose(1, 2))[0]
    print("WNConfig, T = 32: fp32 ring oracle against fp64, worst row %.3e" % e)
    assert 0 < e < 64 * 2.0 ** -23            # a few hundred fp32 roundings deep, far from 1e-4; and the two runs do differ
    assert (o32.double() - o64).abs().max() < 1e-5
    # the inputs were not cast in place
    assert sd["first_conv.weight_v"].dtype == torch.float32 and cg.dtype == torch.float32


def test_ring_oracle_one_hot_input_reproduces_the_reference_golden(golden_dir):
    """the one-hot network through the ring form, fp32 default: the reference's teacher-forced probabilities and logits, its free-running probabilities, and
    every class of its sampled run (inverse cdf with the injected uniform; the fixture keeps every draw >= 1e-4 from an edge)"""
    gold = np.load(os.path.join(golden_dir, "wavenet_onehot_synth.npz"))
    name, cfg, tag = "small", W.WNConfigOneHot, "WN."
    B, T, K, stride, utag = (int(v) for v in gold[name + ".meta"])
    sd = W.wavenet_state(cfg, tag)
    sd["first_conv.weight_g"] = sd["first_conv.weight_g"] * float(gold[name + ".gains"][0])
    sd["last_conv_layers.3.weight_g"] = sd["last_conv_layers.3.weight_g"] * float(gold[name + ".gains"][1])
    c = O.cf_uniform("wnos.%s.c" % name, (B, cfg.cin_channels, T // 16), 0, 1)
    idx = (O.cf_uniform("wnos.%s.idx" % name, (B, T), 0, 1) * K).long().clamp(max=K - 1)
    x = torch.nn.functional.one_hot(idx, K).float().transpose(1, 2).contiguous()
    u = O.cf_uniform("wnos.%s.u%d" % (name, utag), (1, T), 0, 1)
    p, lg = W.incremental_forward_ring(sd, c, T, None, None, cfg, test_inputs=x, softmax=True, quantize=False, return_logits=True)
    assert tuple(p.shape) == (B, K, T) and relerr(p[:, :, ::stride], gold[name + ".p_tf"]) < 1e-5
    assert relerr(lg[:, :, torch.from_numpy(gold[name + ".logit_steps"])], gold[name + ".l_tf"]) < 1e-5
    assert torch.equal(W.incremental_forward_ring(sd, c, T, None, None, cfg, test_inputs=idx, softmax=True, quantize=False), p)      # integer classes
    pf = W.incremental_forward_ring(sd, c, T, None, None, cfg, test_inputs=x[:, :, :4], softmax=True, quantize=False)
    assert relerr(pf[:, :, ::stride], gold[name + ".p_free"]) < 1e-3
    for dt in (None, torch.float64):
        cls = W.incremental_forward_ring(sd, c[:1], T, None, u, cfg, test_inputs=x[:1, :, :4], return_classes=True, dtype=dt)
        assert torch.equal(cls.reshape(T), torch.from_numpy(gold[name + ".classes"])), dt
    hot = W.incremental_forward_ring(sd, c[:1], T, None, u, cfg, test_inputs=x[:1, :, :4])
    assert torch.equal(hot.argmax(1), cls) and torch.equal(hot.sum(1), torch.ones(1, T))


# -------------------------------------------------------------------------------------------------------------------- 2. the measure's worth
def test_per_row_measure_catches_localized_defects_the_aggregate_measure_averages_away():
    """`ragged`, B = 4, teacher-forced: the fp32 restatement with one deliberate defect at a time against the fp64 truth.
    (a) one row of one layer's conv1x1_out zeroed (weight and bias); (b) one stream's ring read one slot late on one layer (the oldest tap of layer 1 taken
    from the middle tap's slot neighbour); (c) the conditioning frame index off by one at the last step only."""
    r = S.Run("ragged", "unfused", 4, ())
    cfg, sd = S.state(r.net)
    d = S.inputs(r)
    T = d["T"]
    truth = S.oracle_logits(r.net, sd, d, d["x"], torch.float64)
    clean = S.oracle_logits(r.net, sd, d, d["x"], None)
    yard = S.worst_row(clean, truth)[0]
    bound = S.MARGIN * yard
    print("ragged B4 T%d: clean fp32 worst row %.3e, bound %.3e, clean Frobenius %.3e" % (T, yard, bound, S.frobenius(clean, truth)))

    sd_a = dict(sd)
    g = sd["conv_layers.1.conv1x1_out.weight_g"].clone(); g[17] = 0
    b = sd["conv_layers.1.conv1x1_out.bias"].clone(); b[17] = 0
    sd_a["conv_layers.1.conv1x1_out.weight_g"], sd_a["conv_layers.1.conv1x1_out.bias"] = g, b
    bad_a = S.oracle_logits(r.net, sd_a, d, d["x"], None)

    # stream 2, layer 1 (d = 2, ring of 5 slots): the hook sees the gathered taps, so "one slot late" is restated on them -- the oldest tap of step t
    # (slot t - 2d) is replaced by the oldest tap of step t + 1 (slot t - 2d + 1), recorded in a clean run first
    taps = {}

    def record(t, layer, x):
        if layer == 1:
            taps[t] = x[2, 0].clone()
        return x
    S.oracle_logits(r.net, sd, d, d["x"], None, tap_hook=record)

    def one_slot_late(t, layer, x):
        if layer != 1 or t + 1 not in taps:
            return x
        x = x.clone()
        x[2, 0] = taps[t + 1]
        return x
    bad_b = S.oracle_logits(r.net, sd, d, d["x"], None, tap_hook=one_slot_late)

    d_c = dict(d)
    c = d["c"].clone(); c[:, :, T - 1] = c[:, :, T - 2]
    d_c["c"] = c
    bad_c = S.oracle_logits(r.net, sd, d_c, d["x"], None)

    for what, bad in (("(a) one conv1x1_out row zeroed", bad_a), ("(b) one stream's ring read one slot late", bad_b), ("(c) conditioning frame off by one at the last step", bad_c)):
        e, bb, tt, ch = S.worst_row(bad, truth)
        print("%-52s worst row %.3e (stream %d, step %d) = %.0f x bound;  Frobenius-relative over the tensor %.3e" % (what, e, bb, tt, e / bound, S.frobenius(bad, truth)))
        assert e > bound, (what, e, bound)
    assert S.worst_row(bad_b, truth)[1] == 2 and S.worst_row(bad_c, truth)[2] == T - 1


# ----------------------------------------------------------------------------------------------------------------------- 3. branch coverage
def test_runs_cover_both_sides_of_every_switch():
    """host only, nothing launched: over RUNS (plus the pipelined runs at the reference size, B = 1 and 3) every switch of a synthesis time step is taken both ways"""
    sws = [(r, *S.switches(r)) for r in S.RUNS]
    kernels = set()
    for r, sw, k in sws:
        kernels |= {n.split("<")[0].split("(")[0] for n in k}
        print("%-34s %-13s %s" % (S.run_id(r), sw["head"], " ".join(k)))
    assert kernels == {"wn_first_kernel", "wn_gate_kernel", "wn_out_kernel", "wn_head_kernel", "wn_head_generic_kernel", "wn_tick_kernel", "wn_stage_kernel",
                       "wn_head_fused_kernel", "wn_head_rows_kernel", "wn_head_sample_kernel", "wn_cat_first_kernel", "wn_cat_rows_kernel", "wn_cat_sample_kernel"}
    val = lambda key, pred=lambda r, sw: True: {sw[key] for r, sw, k in sws if pred(r, sw)}
    assert val("fused") == {True, False}
    assert val("refused_by") >= {"S", "H"}                                   # wn_fused_ok says no for either reason (out_ch > 256 has no kernel past the generic head's)
    for fam in (lambda r, sw: not sw["fused"] and not sw["device_t"], lambda r, sw: sw["fused"] and not sw["device_t"], lambda r, sw: sw["device_t"]):
        assert val("NB", fam) == {1, 2, 4, 8}
        assert val("categorical", fam) == {True, False}
    assert val("head") == {"head", "head_generic", "rows+sample", "head_fused", "cat"}
    for fused in (True, False):
        assert val("cat_first", lambda r, sw: sw["categorical"] and sw["fused"] == fused) >= {"class", "dense"}
        assert val("device_t", lambda r, sw: sw["fused"] == fused) == {True, False}
        assert val("n", lambda r, sw: sw["fused"] == fused) == {"1", "2", ">2"}       # l == 0 / first_skip / last layer: alone, adjacent, apart
        assert val("cond", lambda r, sw: sw["fused"] == fused) == {"local", "+global", "local+global", ""}
        assert True in val("mask", lambda r, sw: sw["fused"] == fused)
    assert "mixed" in val("cat_first")
    # every ring wraps twice
    for r, sw, k in sws:
        assert S.length(r.net) >= 2 * (2 * max(S.dilations(r.net)) + 1) + 5
    assert max(max(S.dilations(r.net)) for r in S.RUNS) == 32
    # reduction lengths with remainders: 3C no multiple of 256 chunks' 1024 floats, H no multiple of 64
    C, G, Sk, cin = S.NETS["ragged"][:4]
    assert (3 * C) % 256 != 0 and (G // 2) % 64 != 0 and (C + Sk) % 4 == 0 and 3 * C + cin > 256 and (3 * C + G // 2 + cin) // 4 > 64


# ------------------------------------------------------------------------------------------------------------------- 4. categorical draws
@pytest.mark.parametrize("K", S.CAT_KS)
def test_categorical_edge_draws_are_all_decisive(K):
    for kind, row in S.cat_rows(K).items():
        u, cls, dropped = S.cat_edge_uniforms(row)
        cdf = S.cat_cdf64(row)
        print("K = %3d %-7s %2d draws, classes %s, dropped %d" % (K, kind, u.numel(), sorted(set(cls.tolist())), dropped))
        assert dropped == 0
        assert u.numel() >= 4 and float(u.min()) >= 0.0 and float(u.max()) < 1.0
        if kind != "peaked":
            assert float(u.min()) == 0.0 and float(u.max()) == float(np.float32(1.0 - 1e-7))
            assert {0, K - 1} <= set(cls.tolist())
            # a draw on either side of the first and of the last edge
            for k in (0, K - 2):
                assert ((u.double().numpy() < cdf[k]) & (u.double().numpy() > cdf[k] - 2 * S.EDGE_OFF)).any() or cdf[k] < S.EDGE_OFF
                assert ((u.double().numpy() > cdf[k]) & (u.double().numpy() < cdf[k] + 2 * S.EDGE_OFF)).any()
        else:
            assert set(cls.tolist()) == {K // 2}                             # every draw between the two edge clusters is the peak
        # the class is the oracle's draw
        p = torch.softmax(row.double(), 0).reshape(1, K).expand(u.numel(), K)
        assert torch.equal(W.categorical_draw(p, u), cls)
