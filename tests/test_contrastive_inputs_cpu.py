"""The inputs of tests/test_contrastive_pipeline_passes_gpu.py, checked without a GPU (tests/contrastive_common.py: the truths, the builders, THE
CONDITION).  For every case the GPU file uses:

  * every decision margin exceeds COND (64) x the fp32 restatement's worst error on the quantity compared, so the fp32 restatement takes every
    hinge, arg-max and rank decision as fp64 does (asserted too), and a kernel that decides otherwise is wrong, not unlucky;
  * the planted ties are exact in fp32: equal rows are equal bit for bit, their scores / squared distances are equal bit for bit, the planted
    zero distances are +0;
  * each margin kind does what its name says (no hinge active / one row without / part / all), and the planted tie is the maximum of its row;
  * the closed-form gradient equals fp64 autograd of the oracle wherever no distance is zero."""
import numpy as np
import pytest
import torch

import contrastive_common as C
from oracle import pipeline_oracle as P


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("n,d", C.L2C_SHAPES)
def test_l2c_case_meets_the_condition(n, d):
    f1, f2, s64, s32, err = C.l2c_scores(n, d)
    pl = C.l2c_plan(n)
    off = ~torch.eye(n, dtype=torch.bool)
    for kind, (m, e, hinge, top2) in C.l2c_condition(n, d).items():
        print("n=%d d=%d %-4s margin %.7g  fp32 score error %.2e  hinge margin %.2e  top-two margin %.2e" % (n, d, kind, m, e, hinge, top2))
        assert m == C.f32(m) and e == err
        assert hinge > C.COND * err and top2 > C.COND * err, (kind, m, err, hinge, top2)
        act = ((m - s64) > 0) & off
        if kind == "zero":
            assert not bool(act.any())
            assert float(C.l2c_ref64(f1, f2, s64, m, 0)["loss"]) == float((s64.diag() ** 2).sum() / (2 * n))
        elif n > 1:
            rows = act.any(1)
            if kind == "row":
                assert int((~rows).sum()) == 1 and (pl is None or not bool(rows[pl["far"]]))
            if kind == "mid":
                assert bool(act.any()) and not bool(act[off].all())
            if kind == "all":
                assert bool(act[off].all())
        for mv in (0, 1):
            W64, a64, c64 = C.weights(s64, m, mv)
            W32, a32, c32 = C.weights(s32, m, mv)
            assert np.array_equal(a64, a32)
            assert bool(((W64 != 0) == (W32 != 0)).all())
        if pl is not None and kind in ("mid", "all"):
            a64 = C.argmax_rows(s64, m)
            assert a64[pl["a0"]] == pl["p"] and float(m - s64[pl["a0"], pl["p"]]) > 0           # the planted tie is its row's maximum; the lower index
            assert a64[pl["x"]] == pl["y"]                                                        # the zero distance costs the whole margin
            assert float(C.weights(s64, m, 1)[0][pl["x"]][off[pl["x"]]].abs().sum()) == 0.0       # ... and its row then has no hinge gradient at all
    if n == 1:
        assert C.argmax_rows(s64, 1.0).tolist() == [-1]


@pytest.mark.parametrize("n,d", [c for c in C.L2C_SHAPES if c[0] >= 5])
def test_l2c_planted_ties_are_exact_in_fp32(n, d):
    f1, f2, s64, s32, _ = C.l2c_scores(n, d)
    pl = C.l2c_plan(n)
    assert len({pl["a0"], pl["z"], pl["x"], pl["far"]}) == 4 and len({pl["p"], pl["q"], pl["z"], pl["y"]}) == 4 and pl["p"] < pl["q"]
    assert torch.equal(_bits(f2[pl["p"]]), _bits(f2[pl["q"]]))
    assert torch.equal(_bits(f2[pl["z"]]), _bits(f1[pl["z"]])) and torch.equal(_bits(f2[pl["y"]]), _bits(f1[pl["x"]]))
    for s in (s32, s64):
        assert torch.equal(s[:, pl["p"]], s[:, pl["q"]])
        assert float(s[pl["z"], pl["z"]]) == 0.0 and float(s[pl["x"], pl["y"]]) == 0.0
        assert int((s == 0).sum()) == 2
    assert int(_bits(s32[pl["z"], pl["z"]].reshape(1))) == 0 and int(_bits(s32[pl["x"], pl["y"]].reshape(1))) == 0
    # the far row really is beyond every other distance
    assert float(s64[pl["far"]].min()) > float(torch.cat([s64[:pl["far"]], s64[pl["far"] + 1:]]).max()) or d == 1


@pytest.mark.parametrize("n,d", C.L2C_SHAPES)
def test_closed_form_gradient_matches_fp64_autograd(n, d):
    f1, f2 = C.l2c_inputs(n, d, ties=True, zeros=False)
    s64 = C.scores_of(f1, f2, torch.float64)
    pl = C.l2c_plan(n)
    for kind in C.MARGIN_KINDS:
        m = C.l2c_margin(s64, kind)
        for mv in (0, 1):
            e = C.closed_form_vs_autograd(f1, f2, m, mv, merge=None if pl is None else (pl["p"], pl["q"]))
            print("n=%d d=%d %-4s mv=%d closed form vs autograd: %.2e of the largest entry" % (n, d, kind, mv, e))
            assert e <= 1e-12, (kind, mv, e)


@pytest.mark.parametrize("case", C.RET_CASES, ids=lambda c: "%d-%d-%d-%s" % c)
def test_retrieval_case_meets_the_condition(case):
    n_clips, n_cap, dim, family = case
    clips, caps, d64, d32, err = C.ret_truth(*case)
    e, rank, top2 = C.ret_condition(*case)
    print("clips %d captions %d dim %d %s: fp32 d2 error %.2e  rank margin %.2e  top-two margin %.2e" % (n_clips, n_cap, dim, family, e, rank, top2))
    assert C.ret_condition_holds(*case)
    if family == "g":
        assert err == 0.0 and torch.equal(d32.double(), d64)
        assert torch.equal(clips * 8, torch.round(clips * 8)) and torch.equal(caps * 8, torch.round(caps * 8))
        assert float(clips.abs().max()) <= 1.0 and float(caps.abs().max()) <= 1.0
    else:
        assert rank > C.COND * err and top2 > C.COND * err
    r64, t64 = C.ret_decisions(d64)
    r32, t32 = C.ret_decisions(d32)
    assert np.array_equal(r64, r32) and np.array_equal(t64, t32)
    _, ranks, top1 = P.l2_retrieval(clips.numpy(), caps.numpy())                    # the oracle: a stable sort of the fp64 distances
    assert np.array_equal(ranks, r64) and np.array_equal(top1, t64)
    pl = C.ret_plan(n_clips, n_cap)
    if pl is not None:
        i0, i1 = pl["i0"], pl["i1"]
        assert pl["jl"] < i0 < pl["jh"] and pl["k1"] < pl["k2"]
        for d2 in (d32, d64):
            assert float(d2[i0, pl["jl"]]) == float(d2[i0, i0]) == float(d2[i0, pl["jh"]])
            assert torch.equal(d2[:, pl["k1"]], d2[:, pl["k2"]])
        assert torch.equal(_bits(clips[pl["jl"]]), _bits(clips[i0])) and torch.equal(_bits(clips[pl["jh"]]), _bits(clips[i0]))
        assert torch.equal(_bits(clips[pl["k1"]]), _bits(clips[pl["k2"]]))
        # the lower copy counts towards the rank, the upper does not; the duplicated nearest clip is top-1 by its lower index
        strictly = int((d64[i0] < d64[i0, i0]).sum())
        below = int((d64[i0, :i0] == d64[i0, i0]).sum())
        assert below >= 1 and r64[i0] == strictly + below
        assert float(d64[i1, pl["k1"]]) == float(d64[i1].min()) and t64[i1] <= pl["k1"]
        assert t64[i1] == pl["k1"] or dim == 1                                      # (17 grid levels at dim = 1: an earlier clip may sit there too)
    if family == "g" and n_clips >= 255:
        assert len(set(r64.tolist())) > 20                                          # the ranks spread; natural ties abound
