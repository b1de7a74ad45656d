"""BatchNorm passes (csrc/bn.hip) called directly at the C ABI and compared with fp64 statistics / fp64 autograd on the CPU
(tests/passes_common.py: how the bounds are made).  nn.BatchNorm2d semantics: biased variance for the normalisation, unbiased for
running_var, momentum 0.1, eps 1e-5.

Branch table -- one row per launch, the parametrisation that reaches each branch.  Streaming grids (stream_grid): 256-thread blocks capped at
2048 (stride 524288 quads), 1024-thread blocks capped at 256 when the pass publishes an abs-max (stride 262144 quads); the 4x-unrolled main
loop runs only for n4 > 3 stride.

  launch                               branch                                                     reached by
  bn_finalize_kernel<256>              uniform rows, nblk = 1, 2, 255, 257 (tail loop only)       test_finalize_uniform nblk; last_n = 1 and full
                                       nblk = 1025 (unrolled loop: b + 768 < nblk)                test_finalize_uniform 1025
                                       M = 1                                                      test_finalize_single_sample
                                       NULL gamma / beta / running buffers / nbt                  test_finalize_uniform bare=True
                                       tiles clipped at the map edge (8x8 on 13x21, N = 2)        test_finalize_tiles
                                       per persistent block, one item each (th < 0)               test_finalize_lin C = 64, M = 128 * 4 * 3
                                       per persistent block, blocks 0 walks two items             test_finalize_lin C = 256, M = 128 * 257 (default grid of 256)
                                       viai_bn_finalize_lin without merged parts                  test_finalize_lin C = 32, M = 128 * 5; M % 128 refused
  bn_finalize_kernel<1024>             nblk = 4097 (> 4096), unrolled loop + tail                 test_finalize_uniform 4097 (C = 4)
                                       tiles form with nblk > 4096                                 not run: same kernel body as the two rows above (count() is shared)
  bn_eval_coeffs_kernel                                                                            covered by tests/test_kernels_gpu.py (eval-mode forward)
  bn_act_fwd_kernel<ACT,FIXED,RES,NT>  every ACT x FIXED (C = 32) / non-FIXED (C = 24, 96) x RES   test_apply_fwd_small (M = 37, uncapped)
                                       x NT (amax or not)
                                       capped, tail loop only (stride < n4 < 3 stride)            test_apply_fwd_large size="capped"
                                       capped, unrolled loop + ragged tail (n4 ~ 4 stride + 3 NT)  test_apply_fwd_large size="unrolled"; C = 28 too at NT = 1024,
                                                                                                  where stride % (C/4) differs from NT % (C/4)
  bn_bwd_reduce_kernel<false>          rows_min = 4096 / C, one block, idle lanes                  test_bwd (5, 4)
                                       C/4 = 6, 24 do not divide 256 (idle lanes), short last     test_bwd (1027, 24), (4097, 96)
                                       C/4 = 128 (two pixel lanes)                                test_bwd (513, 512)
                                       512 row blocks, short last one                             test_bwd (66000, 32)
  bn_bwd_final_kernel                  nblk < 64 / > 256 (unrolled walk); training bit 0, bit 1   test_bwd shapes x mode in {train, eval, train+accumulate}
                                       dy = NULL (sums only)                                      test_bwd_sums_only
  bn_bwd_apply_kernel<ACT,FIXED,false> all four activations, uncapped                             test_bwd (act rotates over the shapes, sigmoid included)
                                       capped + unrolled, non-FIXED, NT = 256 (no amax)           test_bwd_large (87414, 96)
                                       capped + unrolled, non-FIXED, NT = 1024 (amax)             test_bwd_large (150237, 28)
  bn_pool_bwd_reduce_kernel            k == 3: sums from the pooled side                          test_pool_bwd (3,2,1) on 8x12 and 9x11, (3,1,1) on 5x7
  bn_bwd_reduce_kernel<true>           any other window                                           test_pool_bwd (2,2,0) on 8x8x24
  bn_pool2x2_bwd_apply_kernel          (3,2,1) on an even map                                     test_pool_bwd (3,2,1) on 2x8x12x32
  bn_bwd_apply_kernel<ACT,FIXED,true>  generic gather: odd map; non-FIXED; overlapping windows     test_pool_bwd 9x11x32, 8x8x24, 5x7x32; one / two addends
  bn_bwd_reduce_kernel<false,true>     MAXDP partial (the P16 bound)                              test_bwd_p16 p16 / twin
  bn_bwd_reduce_kernel<false,true,true> JOIN: masked sum of one / two addends written to dres      test_bwd_p16 join (uncapped: two addends, capped: one)
  bn_bwd_final_kernel ps = 3           the bound sums[2C + c]                                      test_bwd_p16: published amax against the fp64 formula
  bn_bwd_apply_p16_kernel<FIXED>       C = 32 (FIXED) / 96; uncapped (M = 517); capped + 2x-unrolled test_bwd_p16 sizes (n8 = 2 stride + 261 octets at the large one);
                                       loop + tail; dy32 twin                                      decoded with viai_p16_decode, against fp64 autograd
  p16_decode_kernel                    uncapped / capped grid                                      every P16 case here decodes through it
  bn_act_fwd_p16_kernel<FIXED>         C = 32 / 96; uncapped / capped + 2x-unrolled                test_apply_fwd_p16
  bn_add_act_twin_kernel<ACT>          uncapped / capped + 4x-unrolled (C = 32, 64)                test_add_act_twin
  act_bwd_out_kernel                   all four activations; n > 8192 * 256 (grid wraps)          tests/test_pool_passes_gpu.py::test_act_bwd_from_output
  add_act_bwd_out_kernel                                                                           tests/test_pool_passes_gpu.py::test_join_passes
  M * C >= 2^31 (pool-fused reduce falls back to the generic kernel)                               not run: 8 GB per tensor
"""
import os

import pytest
import torch
import torch.nn.functional as F

from passes_common import (EPS32, INVALID, LRELU, NONE, RELU, SIGMOID, SLOPE, ACT_IDS, act64, assert_bitwise, bound_abs, check_abs, check_p16, dev, host,
                           lib, ok, ptr, st, uniform)

pytestmark = pytest.mark.gpu

BN_EPS, MOMENTUM = 1e-5, 0.1

# worst error measured on the MI355X per pass family (bounds are made per case: passes_common / _finalize_bounds)
MEASURED = {       # worst (error / bound) over the cases, and that case's error
    "finalize (all forms, every output)": "0.26 of the bound (running_mean, lin C = 256); mean 1.7e-5 abs on the 1e3-mean channel at nblk = 4097",
    "apply forward": "0.25 of the bound = the fp32 restatement's own error: 3.6e-7 on 4.3 (M = 262241, C = 32, res)",
    "backward dgamma / dbeta": "0.44 of the bound: 5.1e-6 on 32 at (1027, 24) relu train",
    "backward dy": "0.26 of the bound: 1.2e-7 on 1.3 at (66000, 32)",
    "pool-fused backward dgamma / dbeta": "0.85 of the bound: 2.4e-6 on 11.8 (dbeta, k3 s2 p1 2x8x12x32 relu, two addends: the 2-ulp floor)",
    "pool-fused backward dy": "0.35 of the bound: 3.6e-7 on 3.6",
    "P16 backward (p16 / twin / join), decoded dy": "0.21 of value bound + storage error: 4.0e-7 with planes bounded by 3.1 (join, (517, 32))",
    "P16 forward / add_act twin, decoded z": "0.24: 3.6e-7 with planes bounded by 3.3 / 6.9e-7 with 4.3",
}


# ---------------------------------------------------------------- finalize

def _channel_data(tag, M, Cc):
    """(M, C) fp32: unit-spread noise around per-channel means of 0, 1, 30 and 1e3 times the spread"""
    mean = torch.tensor([0.0, 1.0, -30.0, 1000.0]).repeat((Cc + 3) // 4)[:Cc]
    return (uniform(tag, (M, Cc)).double() * 1.7 + mean.double()).float()


def _stats64(x):
    """fp64 statistics of the fp32 tensor itself: mean, biased variance, unbiased variance (M = 1: the biased one, as the kernel keeps it)"""
    x = x.double()
    M = x.shape[0]
    mean = x.mean(0)
    m2 = ((x - mean) ** 2).sum(0)
    return mean, m2 / M, (m2 / (M - 1) if M > 1 else m2 / M)


def _partials(groups, Cc):
    """groups: list of (n_b, C) fp64 blocks -> (mean_b, M2_b) in fp64, (nblk, C) each"""
    mb = torch.stack([g.mean(0) for g in groups])
    m2 = torch.stack([((g - g.mean(0)) ** 2).sum(0) for g in groups])
    return mb, m2


def _pack(mb, m2):
    """the layout of every form: part[c * nblk + b] = mean, part[(C + c) * nblk + b] = M2, rounded to fp32"""
    return torch.cat([mb.t().contiguous().reshape(-1), m2.t().contiguous().reshape(-1)]).float()


def _finalize_bounds(x, mb, m2, counts, gamma, beta, rm, rv):
    """Bounds of every output from what went IN: the fp32 rounding of the result (2 ulp allowed) plus the effect of rounding the block partials to
    fp32 (relative 2^-24 each): d mean <= 2^-24 max|m_b|;  d M2 <= 2^-24 sum(M2_b) + 2 sum n_b |m_b - mean| d m_b + sum n_b d m_b^2."""
    M = x.shape[0]
    mean, var, unb = _stats64(x)
    h = 2.0 ** -24
    dmb = h * mb.abs()
    n = counts.double()[:, None]
    d_mean = (n * dmb).sum(0) / M
    d_m2 = h * m2.sum(0) + 2 * (n * (mb - mean).abs() * dmb).sum(0) + (n * dmb * dmb).sum(0)
    d_var = d_m2 / M
    invstd = 1.0 / torch.sqrt(var + BN_EPS)
    t_mean = d_mean + 2 * EPS32 * mean.abs()
    t_invstd = 0.5 * invstd ** 3 * d_var * 1.01 + 2 * EPS32 * invstd
    g, b = gamma.double(), beta.double()
    t_scale = g.abs() * t_invstd + 2 * EPS32 * (g * invstd).abs()
    t_shift = g.abs() * (mean.abs() * t_invstd + invstd * t_mean) + 3 * EPS32 * (b.abs() + (mean * g * invstd).abs())
    t_rm = MOMENTUM * t_mean + 3 * EPS32 * (rm.double().abs() + mean.abs())
    t_rv = MOMENTUM * d_var * (M / max(M - 1, 1)) + 3 * EPS32 * (rv.double().abs() + unb.abs())
    ref = {"mean": mean, "invstd": invstd, "scale": g * invstd, "shift": b - mean * g * invstd,
           "running_mean": (1 - MOMENTUM) * rm.double() + MOMENTUM * mean, "running_var": (1 - MOMENTUM) * rv.double() + MOMENTUM * unb}
    tol = {"mean": t_mean, "invstd": t_invstd, "scale": t_scale, "shift": t_shift, "running_mean": t_rm, "running_var": t_rv}
    return ref, tol


def _check_finalize(what, x, mb, m2, counts, call, bare=False):
    """call(part, gamma, beta, rm, rv, nbt, mean, invstd, scale, shift) -> hipError_t; compares every output with the tensor's own fp64 statistics"""
    M, Cc = x.shape
    assert int(counts.sum()) == M
    gamma, beta = uniform("fin.g", (Cc,), 0.5, 1.5), uniform("fin.b", (Cc,), -0.5, 0.5)
    rm, rv = uniform("fin.rm", (Cc,), -1.0, 1.0), uniform("fin.rv", (Cc,), 0.5, 2.0)
    if bare:
        gamma, beta = torch.ones(Cc), torch.zeros(Cc)
    ref, tol = _finalize_bounds(x, mb, m2, counts, gamma, beta, rm, rv)
    part = dev(_pack(mb, m2))
    gd, bd, rmd, rvd = dev(gamma), dev(beta), dev(rm), dev(rv)
    nbt = torch.tensor([41], dtype=torch.int64, device="cuda")
    outs = [torch.full((Cc,), float("nan"), device="cuda") for _ in range(4)]
    if bare:
        ok(call(part, None, None, None, None, None, *outs), what)
    else:
        ok(call(part, gd, bd, rmd, rvd, nbt, *outs), what)
    got = dict(zip(("mean", "invstd", "scale", "shift"), outs))
    if not bare:
        got["running_mean"], got["running_var"] = rmd, rvd
        assert int(nbt) == 42
    else:
        assert int(nbt) == 41
    for k, v in got.items():
        err = (host(v).double() - ref[k]).abs()
        worst = float((err / tol[k]).max())
        print("%-34s %-13s worst err / bound %.3f  (max err %.3e)" % (what, k, worst, float(err.max())))
        assert bool((err <= tol[k]).all()), (what, k, worst)


def _uniform_case(nblk, last_n, Cc, rows=3):
    M = (nblk - 1) * rows + last_n
    x = _channel_data("fin.x", M, Cc)
    groups = list(torch.split(x.double(), rows))
    assert len(groups) == nblk and groups[-1].shape[0] == last_n
    mb, m2 = _partials(groups, Cc)
    counts = torch.tensor([g.shape[0] for g in groups])
    return x, mb, m2, counts


@pytest.mark.parametrize("bare", [False, True], ids=["affine", "bare"])
@pytest.mark.parametrize("last_n", [1, 3])
@pytest.mark.parametrize("nblk", [1, 2, 255, 257, 1025, 4097])
def test_finalize_uniform(nblk, last_n, bare):
    L = lib()
    Cc, rows = 4, 3
    x, mb, m2, counts = _uniform_case(nblk, last_n, Cc, rows)
    M = x.shape[0]

    def call(part, g, b, rm, rv, nbt, mean, invstd, scale, shift):
        return L.viai_bn_finalize(part.data_ptr(), nblk, rows, M, Cc, ptr(g), ptr(b), ptr(rm), ptr(rv), ptr(nbt), MOMENTUM, BN_EPS,
                                  mean.data_ptr(), invstd.data_ptr(), scale.data_ptr(), shift.data_ptr(), st())
    _check_finalize("finalize nblk=%d last=%d" % (nblk, last_n), x, mb, m2, counts, call, bare)


def test_finalize_single_sample():
    """M = 1: variance 0, invstd = 1 / sqrt(eps); running_var takes the biased variance (torch refuses to train on one value per channel)"""
    L = lib()
    Cc = 8
    x, mb, m2, counts = _uniform_case(1, 1, Cc, rows=1)

    def call(part, g, b, rm, rv, nbt, mean, invstd, scale, shift):
        return L.viai_bn_finalize(part.data_ptr(), 1, 1, 1, Cc, ptr(g), ptr(b), ptr(rm), ptr(rv), ptr(nbt), MOMENTUM, BN_EPS,
                                  mean.data_ptr(), invstd.data_ptr(), scale.data_ptr(), shift.data_ptr(), st())
    _check_finalize("finalize M=1", x, mb, m2, counts, call)
    z = torch.zeros(4, device="cuda")
    for bad in ((0, 1, 1, Cc), (1, 1, 0, Cc), (1, 1, 1, 0)):
        assert L.viai_bn_finalize(z.data_ptr(), bad[0], bad[1], bad[2], bad[3], 0, 0, 0, 0, 0, MOMENTUM, BN_EPS,
                                  z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), st()) == INVALID


def test_finalize_tiles():
    """8 x 8 tiles on a 13 x 21 map: every tile of the last tile row / column is clipped (5 rows, 5 columns)"""
    L = lib()
    N, OH, OW, th, tw, Cc = 2, 13, 21, 8, 8, 8
    x = _channel_data("fin.tiles", N * OH * OW, Cc)
    x4 = x.double().reshape(N, OH, OW, Cc)
    groups = [x4[n, ty:ty + th, tx:tx + tw].reshape(-1, Cc) for n in range(N) for ty in range(0, OH, th) for tx in range(0, OW, tw)]
    assert sorted(set(g.shape[0] for g in groups)) == [25, 40, 64]
    mb, m2 = _partials(groups, Cc)
    counts = torch.tensor([g.shape[0] for g in groups])

    def call(part, g, b, rm, rv, nbt, mean, invstd, scale, shift):
        return L.viai_bn_finalize_tiles(part.data_ptr(), N, OH, OW, th, tw, Cc, ptr(g), ptr(b), ptr(rm), ptr(rv), ptr(nbt), MOMENTUM, BN_EPS,
                                        mean.data_ptr(), invstd.data_ptr(), scale.data_ptr(), shift.data_ptr(), st())
    _check_finalize("finalize tiles 8x8 on 13x21", x, mb, m2, counts, call)


@pytest.mark.parametrize("Cc,items128", [(32, 5), (64, 12), (256, 257)])
def test_finalize_lin(Cc, items128):
    """viai_bn_finalize_lin: partials per 128 pixels (C = 32: no merged parts), or merged per persistent block of the linear-tile conv kernel --
    part b = (block b / PW, sub-block b % PW) holds the pixels [128 (item PW + b % PW), + 128) of every item the block walked (items blk, blk + G, ..).
    C = 64 (PW = 4): 3 items on 3 blocks, one each.  C = 256 (PW = 1): 257 items on the default grid of 256 blocks, so block 0 holds items 0 and 256."""
    L = lib()
    assert os.environ.get("VIAI_DMA_GRID") in (None, "256") and os.environ.get("VIAI_LIN_STAT_MERGE") in (None, "1"), \
        "this test lays the partials out for the library's defaults (256 persistent blocks, merged parts): unset VIAI_DMA_GRID / VIAI_LIN_STAT_MERGE"
    M = 128 * items128
    x = _channel_data("fin.lin", M, Cc)
    chunks = list(torch.split(x.double(), 128))
    if Cc == 256:
        groups = [torch.cat([chunks[0], chunks[256]])] + chunks[1:256]
    else:
        groups = chunks
    mb, m2 = _partials(groups, Cc)
    counts = torch.tensor([g.shape[0] for g in groups])

    def call(part, g, b, rm, rv, nbt, mean, invstd, scale, shift):
        return L.viai_bn_finalize_lin(part.data_ptr(), M, Cc, ptr(g), ptr(b), ptr(rm), ptr(rv), ptr(nbt), MOMENTUM, BN_EPS,
                                      mean.data_ptr(), invstd.data_ptr(), scale.data_ptr(), shift.data_ptr(), st())
    _check_finalize("finalize_lin C=%d M=%d" % (Cc, M), x, mb, m2, counts, call)
    z = torch.zeros(2 * Cc, device="cuda")
    assert L.viai_bn_finalize_lin(z.data_ptr(), M + 1, Cc, 0, 0, 0, 0, 0, MOMENTUM, BN_EPS, z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), st()) == INVALID


# ---------------------------------------------------------------- apply forward

def _coeffs(tag, Cc):
    scale = uniform(tag + ".sc", (Cc,), 0.5, 1.5) * torch.sign(uniform(tag + ".sg", (Cc,)) + 0.7)       # a few negative gammas
    shift = uniform(tag + ".sh", (Cc,), -0.5, 0.5)
    return scale, shift


def _off_kink(y, res, scale, shift, lim=1e-4):
    """move the elements whose pre-activation lies within 2 lim of zero by 8 lim / |scale| (in y); assert that none is left within lim"""
    def pre(v):
        p = v.double() * scale.double() + shift.double()
        return p if res is None else p + res.double()
    near = pre(y).abs() < 2 * lim
    y = torch.where(near, y + (8 * lim / scale.abs()).expand_as(y), y)
    assert bool((pre(y).abs() > lim).all()), "generator left a pre-activation within %g of the kink" % lim
    return y


def _run_apply_fwd(M, Cc, act, with_res, with_amax):
    L = lib()
    scale, shift = _coeffs("af%d" % Cc, Cc)
    res = uniform("af.res", (M, Cc), -1.0, 1.0) if with_res else None
    y = _off_kink(uniform("af.y", (M, Cc), -2.0, 2.0), res, scale, shift)
    pre64 = y.double() * scale.double() + shift.double()
    pre32 = y * scale + shift
    if with_res:
        pre64, pre32 = pre64 + res.double(), pre32 + res
    ref, f32 = act64(pre64, act), act64(pre32, act)
    yd, sd, hd = dev(y), dev(scale), dev(shift)
    z = torch.full((M, Cc), float("nan"), device="cuda")
    am = torch.zeros(1, device="cuda") if with_amax else None
    if with_res:
        rd = dev(res)
        ok(L.viai_bn_add_act_fwd_amax(yd.data_ptr(), sd.data_ptr(), hd.data_ptr(), rd.data_ptr(), z.data_ptr(), M, Cc, act, SLOPE, ptr(am), st()),
           "viai_bn_add_act_fwd_amax")
    elif with_amax:
        ok(L.viai_bn_act_fwd_amax(yd.data_ptr(), sd.data_ptr(), hd.data_ptr(), z.data_ptr(), M, Cc, act, SLOPE, am.data_ptr(), st()), "viai_bn_act_fwd_amax")
    else:
        ok(L.viai_bn_act_fwd(yd.data_ptr(), sd.data_ptr(), hd.data_ptr(), z.data_ptr(), M, Cc, act, SLOPE, st()), "viai_bn_act_fwd")
    check_abs(z, ref, f32, "bn_act_fwd M=%d C=%d act=%s res=%d amax=%d" % (M, Cc, ACT_IDS[act], with_res, with_amax))
    if with_amax:
        assert_bitwise(am, host(z).abs().max().reshape(1), "bn_act_fwd amax")
        assert abs(float(am) - float(ref.abs().max())) <= bound_abs(ref, f32)            # ... and, independently of z, the truth's maximum


@pytest.mark.parametrize("with_amax", [False, True], ids=["nt256", "nt1024amax"])
@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "res"])
@pytest.mark.parametrize("act", [NONE, RELU, LRELU, SIGMOID], ids=lambda a: ACT_IDS[a])
@pytest.mark.parametrize("Cc", [32, 24, 96])
def test_apply_fwd_small(Cc, act, with_res, with_amax):
    if with_res and act in (LRELU, SIGMOID):
        L = lib()
        t = torch.zeros(37 * Cc, device="cuda")
        assert L.viai_bn_add_act_fwd_amax(t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), 37, Cc, act, SLOPE, 0, st()) == INVALID
        return                                                  # the residual form takes ReLU or none: the refusal is the contract
    _run_apply_fwd(37, Cc, act, with_res, with_amax)


def _large_M(Cc, nt, size):
    """rows for the streaming grid of NT-thread blocks: `capped` lies between stride and 3 stride (tail loop only, 1.3 stride), `unrolled` is
    4 stride + 3 NT + 5 quads rounded up to whole rows; neither is a multiple of the stride"""
    stride = (256 if nt == 1024 else 2048) * nt
    n4 = stride + stride // 3 + 5 if size == "capped" else 4 * stride + 3 * nt + 5
    c4n = Cc // 4
    M = (n4 + c4n - 1) // c4n
    n4 = M * c4n
    assert n4 % stride != 0 and (stride < n4 < 3 * stride if size == "capped" else n4 > 4 * stride)
    return M


@pytest.mark.parametrize("size", ["capped", "unrolled"])
@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "res"])
@pytest.mark.parametrize("Cc,with_amax", [(32, False), (24, False), (96, False), (32, True), (24, True), (96, True), (28, True)])
def test_apply_fwd_large(Cc, with_amax, with_res, size):
    act = RELU if with_res else LRELU
    _run_apply_fwd(_large_M(Cc, 1024 if with_amax else 256, size), Cc, act, with_res, with_amax)


def test_apply_fwd_refuses_ragged_channels():
    L = lib()
    t = torch.zeros(64, device="cuda")
    assert L.viai_bn_act_fwd(t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), 4, 6, RELU, SLOPE, st()) == INVALID


# ---------------------------------------------------------------- backward

def _bn_train_inputs(tag, M, Cc, act):
    """y (fp32, pre-activations clear of the kink), gamma, beta and the fp32-rounded batch statistics the forward would have saved"""
    gamma = uniform(tag + ".g", (Cc,), 0.5, 1.5) * torch.sign(uniform(tag + ".sg", (Cc,)) + 0.7)
    beta = uniform(tag + ".b", (Cc,), -0.5, 0.5)
    y = uniform(tag + ".y", (M, Cc), -2.0, 2.0) + uniform(tag + ".m", (Cc,), -0.5, 0.5)
    for _ in range(3):
        mean, var, _ = _stats64(y)
        invstd = 1.0 / torch.sqrt(var + BN_EPS)
        pre = (y.double() - mean) * invstd * gamma.double() + beta.double()
        near = pre.abs() < 4e-4
        if not bool(near.any()):
            break
        y = torch.where(near, y + 2e-3, y)
    mean, var, _ = _stats64(y)
    invstd = 1.0 / torch.sqrt(var + BN_EPS)
    mean32, invstd32 = mean.float(), invstd.float()
    scale32 = gamma * invstd32
    shift32 = beta - mean32 * scale32
    if act != SIGMOID:
        pre = y.double() * scale32.double() + shift32.double()
        pre_t = (y.double() - mean) * invstd * gamma.double() + beta.double()
        assert bool((pre.abs() > 1e-4).all()) and bool((pre_t.abs() > 1e-4).all()), "generator left a pre-activation near the kink"
    return y, gamma, beta, mean32, invstd32, scale32, shift32


def _bwd_truth(y, dz, gamma, beta, mean32, invstd32, act, training, dtype):
    """autograd of act(BN_train(y)) (training) or of the affine map with the given statistics (eval); dtype fp64 = the truth, fp32 = the scale"""
    yv = y.detach().to(dtype).clone().requires_grad_(True)
    g = gamma.detach().to(dtype).clone().requires_grad_(True)
    b = beta.detach().to(dtype).clone().requires_grad_(True)
    if training:
        mean = yv.mean(0)
        var = ((yv - mean) ** 2).mean(0)
        xhat = (yv - mean) / torch.sqrt(var + BN_EPS)
    else:
        xhat = (yv - mean32.to(dtype)) * invstd32.to(dtype)
    z = act64(xhat * g + b, act)
    z.backward(dz.to(dtype))
    return yv.grad, g.grad, b.grad


def _run_bwd(M, Cc, act, mode, with_amax, with_dy=True):
    L = lib()
    training = {"train": 1, "eval": 0, "train+acc": 3}[mode]
    y, gamma, beta, mean32, invstd32, scale32, shift32 = _bn_train_inputs("bw", M, Cc, act)
    dz = uniform("bw.dz", (M, Cc), -1.0, 1.0)
    dy64, dg64, db64 = _bwd_truth(y, dz, gamma, beta, mean32, invstd32, act, training & 1, torch.float64)
    dy32, dg32, db32 = _bwd_truth(y, dz, gamma, beta, mean32, invstd32, act, training & 1, torch.float32)
    dg0, db0 = uniform("bw.dg0", (Cc,), -3.0, 3.0), uniform("bw.db0", (Cc,), -3.0, 3.0)
    if training & 2:
        dg64, db64, dg32, db32 = dg64 + dg0.double(), db64 + db0.double(), dg32 + dg0, db32 + db0
    nblk = L.viai_bn_bwd_blocks(M, Cc)
    rows = max((M + 511) // 512, max(4, 4096 // Cc))
    assert nblk == (M + rows - 1) // rows
    part = torch.full((2 * Cc * nblk,), float("nan"), device="cuda")
    sums = torch.full((2 * Cc,), float("nan"), device="cuda")
    dg, db = dev(dg0), dev(db0)
    dy = torch.full((M, Cc), float("nan"), device="cuda") if with_dy else None
    am = torch.zeros(1, device="cuda") if with_amax else None
    d = [dev(t) for t in (dz, y, mean32, invstd32, scale32, shift32)]
    ok(L.viai_bn_act_bwd_amax(*[t.data_ptr() for t in d], part.data_ptr(), sums.data_ptr(), dg.data_ptr(), db.data_ptr(), ptr(dy), M, Cc, act, SLOPE,
                              training, ptr(am), st()), "viai_bn_act_bwd_amax")
    what = "bn_bwd (%d, %d) %s %s" % (M, Cc, ACT_IDS[act], mode)
    check_abs(dg, dg64, dg32, what + " dgamma")
    check_abs(db, db64, db32, what + " dbeta")
    if with_dy:
        check_abs(dy, dy64, dy32, what + " dy")
        if with_amax:
            assert_bitwise(am, host(dy).abs().max().reshape(1), what + " amax")
            assert abs(float(am) - float(dy64.abs().max())) <= bound_abs(dy64, dy32)


BWD_SHAPES = [(5, 4, LRELU), (1027, 24, RELU), (4097, 96, SIGMOID), (513, 512, NONE), (66000, 32, LRELU)]


@pytest.mark.parametrize("mode", ["train", "eval", "train+acc"])
@pytest.mark.parametrize("M,Cc,act", BWD_SHAPES, ids=lambda v: str(v))
def test_bwd(M, Cc, act, mode):
    _run_bwd(M, Cc, act, mode, with_amax=(mode != "eval"))


@pytest.mark.parametrize("act", [RELU, SIGMOID], ids=lambda a: ACT_IDS[a])
def test_bwd_every_activation_at_one_ragged_shape(act):
    _run_bwd(1027, 24, act, "train", with_amax=True)
    _run_bwd(1027, 24, {RELU: NONE, SIGMOID: LRELU}[act], "eval", with_amax=False)


def test_bwd_sums_only():
    _run_bwd(1027, 24, LRELU, "train", with_amax=False, with_dy=False)


@pytest.mark.parametrize("M,Cc,with_amax", [(87414, 96, False), (150237, 28, True)])
def test_bwd_large(M, Cc, with_amax):
    """the apply pass capped and inside its unrolled loop with the channel quad changing per iteration (non-FIXED)"""
    assert M == _large_M(Cc, 1024 if with_amax else 256, "unrolled")
    _run_bwd(M, Cc, LRELU, "train", with_amax)


def test_bwd_refuses_ragged_channels():
    L = lib()
    t = torch.zeros(64, device="cuda")
    p = t.data_ptr()
    assert L.viai_bn_act_bwd_amax(p, p, p, p, p, p, p, p, p, p, p, 4, 6, RELU, SLOPE, 1, 0, st()) == INVALID


# ---------------------------------------------------------------- pre-split (P16) producers

def _decode(p16, M, Cc, am):
    out = torch.full((M, Cc), float("nan"), device="cuda")
    ok(lib().viai_p16_decode(p16.data_ptr(), out.data_ptr(), M, Cc, am.data_ptr(), st()), "viai_p16_decode")
    return out


def _p16_M(Cc, size):
    """uncapped: 517 rows; large: 2 stride + 261 octets of the 2048 x 256 grid (the 2x-unrolled loop of the P16 passes, then a ragged tail)"""
    if size == "uncapped":
        return 517
    stride, c8n = 2048 * 256, Cc // 8
    M = (2 * stride + 261 + c8n - 1) // c8n
    assert M * c8n > 2 * stride and (M * c8n) % stride != 0
    return M


@pytest.mark.parametrize("size", ["uncapped", "capped"])
@pytest.mark.parametrize("Cc", [32, 96])
@pytest.mark.parametrize("variant", ["p16", "twin", "join"])
def test_bwd_p16(variant, Cc, size):
    """viai_bn_act_bwd_p16 / _twin / viai_bn_join_bwd_p16: sums against fp64 autograd, the planes decoded against the same truth with the P16 storage
    error on top, the published bound against its formula (include/viai_hip.h) evaluated in fp64"""
    L = lib()
    M = _p16_M(Cc, size)
    act = NONE if variant == "join" else LRELU
    y, gamma, beta, mean32, invstd32, scale32, shift32 = _bn_train_inputs("bw", M, Cc, act)
    dz = uniform("bw.dz", (M, Cc), -1.0, 1.0)
    g64, g32 = dz.double(), dz
    dz2 = zj = None
    if variant == "join":
        zj = uniform("bw.zj", (M, Cc), -1.0, 1.0).clone()
        zj[::5] = 0.0                                              # the join's ReLU output: exact zeros mask the gradient
        mask = (zj > 0).float()
        if size == "uncapped":
            dz2 = uniform("bw.dz2", (M, Cc), -1.0, 1.0)
            g64, g32 = (dz.double() + dz2.double()) * mask.double(), (dz + dz2) * mask
        else:
            g64, g32 = dz.double() * mask.double(), dz * mask
    dy64, dg64, db64 = _bwd_truth(y, g64, gamma, beta, mean32, invstd32, act, 1, torch.float64)
    dy32, dg32, db32 = _bwd_truth(y, g32, gamma, beta, mean32, invstd32, act, 1, torch.float32)
    nblk = L.viai_bn_bwd_blocks(M, Cc)
    part = torch.full((3 * Cc * nblk,), float("nan"), device="cuda")
    sums = torch.full((3 * Cc,), float("nan"), device="cuda")
    dg, db = torch.full((Cc,), float("nan"), device="cuda"), torch.full((Cc,), float("nan"), device="cuda")
    dyp = torch.full((M, Cc), float("nan"), device="cuda")
    am = torch.zeros(1, device="cuda")
    d = [dev(t) for t in (dz, y, mean32, invstd32, scale32, shift32)]
    common = [part.data_ptr(), sums.data_ptr(), dg.data_ptr(), db.data_ptr(), dyp.data_ptr()]
    what = "bn_bwd_%s (%d, %d)" % (variant, M, Cc)
    dy32_out = dres = None
    if variant == "p16":
        ok(L.viai_bn_act_bwd_p16(*[t.data_ptr() for t in d], *common, M, Cc, act, SLOPE, 1, am.data_ptr(), st()), what)
    elif variant == "twin":
        dy32_out = torch.full((M, Cc), float("nan"), device="cuda")
        ok(L.viai_bn_act_bwd_p16_twin(*[t.data_ptr() for t in d], *common, dy32_out.data_ptr(), M, Cc, act, SLOPE, 1, am.data_ptr(), st()), what)
    else:
        dres = torch.full((M, Cc), float("nan"), device="cuda")
        zjd, dz2d = dev(zj), (None if dz2 is None else dev(dz2))
        ok(L.viai_bn_join_bwd_p16(d[0].data_ptr(), ptr(dz2d), zjd.data_ptr(), dres.data_ptr(), *[t.data_ptr() for t in d[1:]], *common, M, Cc, 1,
                                  am.data_ptr(), st()), what)
        assert_bitwise(dres, g32, what + " dres")
    check_abs(dg, dg64, dg32, what + " dgamma")
    check_abs(db, db64, db32, what + " dbeta")
    # the published bound: max over channels of |scale| (max|dpre| + |s2| sqrt(M - 1) / M + |s1| / M) x 1.001, from the fp64 truth
    pre = y.double() * scale32.double() + shift32.double()
    dpre = g64 * (torch.where(pre > 0, torch.ones_like(pre), torch.full_like(pre, SLOPE)) if act == LRELU else 1.0)
    xhat = (y.double() - mean32.double()) * invstd32.double()
    s1, s2 = dpre.sum(0), (dpre * xhat).sum(0)
    want = float((scale32.double().abs() * (dpre.abs().max(0).values + s2.abs() * (M - 1) ** 0.5 / M + s1.abs() / M)).max()) * 1.001
    bound = float(am)
    assert abs(bound - want) <= 1e-5 * want, (what, bound, want)
    assert float(dy64.abs().max()) <= bound
    check_p16(_decode(dyp, M, Cc, am), dy64, dy32, max(bound, want), what + " dy")
    if dy32_out is not None:
        check_abs(dy32_out, dy64, dy32, what + " dy32")


def test_bwd_p16_refusals():
    L = lib()
    t = torch.zeros(256, device="cuda")
    p = t.data_ptr()
    assert L.viai_bn_act_bwd_p16(p, p, p, p, p, p, p, p, p, p, p, 4, 24, RELU, SLOPE, 1, p, st()) == INVALID            # C % 32
    assert L.viai_bn_act_bwd_p16(p, p, p, p, p, p, p, p, p, p, p, 4, 32, SIGMOID, SLOPE, 1, p, st()) == INVALID
    assert L.viai_bn_act_bwd_p16(p, p, p, p, p, p, p, p, p, p, p, 4, 32, RELU, SLOPE, 1, 0, st()) == INVALID            # no amax slot
    assert L.viai_bn_act_bwd_p16_twin(p, p, p, p, p, p, p, p, p, p, p, 0, 4, 32, RELU, SLOPE, 1, p, st()) == INVALID     # no dy32
    assert L.viai_bn_join_bwd_p16(p, 0, 0, p, p, p, p, p, p, p, p, p, p, p, 4, 32, 1, p, st()) == INVALID              # no zj
    assert L.viai_p16_decode(p, p, 4, 24, p, st()) == INVALID


def _fwd_bound(gamma, beta, m_stat):
    return float((gamma.double().abs() * (max(m_stat - 1, 1)) ** 0.5 + beta.double().abs()).max())


@pytest.mark.parametrize("size", ["uncapped", "capped"])
@pytest.mark.parametrize("Cc,act", [(32, LRELU), (96, RELU)])
def test_apply_fwd_p16(Cc, act, size):
    L = lib()
    M = _p16_M(Cc, size)
    scale, shift = _coeffs("af%d" % Cc, Cc)
    y = _off_kink(uniform("af.y", (M, Cc), -2.0, 2.0), None, scale, shift)
    gamma, beta = scale.abs() * 2.0, shift                         # any gamma / beta whose bound covers |z| (|y| <= 2)
    m_stat = 2
    ref = act64(y.double() * scale.double() + shift.double(), act)
    f32 = act64(y * scale + shift, act)
    zp, am = torch.full((M, Cc), float("nan"), device="cuda"), torch.zeros(1, device="cuda")
    d = [dev(t) for t in (y, scale, shift, gamma, beta)]
    ok(L.viai_bn_act_fwd_p16(*[t.data_ptr() for t in d], m_stat, zp.data_ptr(), M, Cc, act, SLOPE, am.data_ptr(), st()), "viai_bn_act_fwd_p16")
    want = _fwd_bound(gamma, beta, m_stat)
    bound = float(am)
    assert want <= bound <= want * 1.0011 and float(ref.abs().max()) <= bound, (bound, want)
    check_p16(_decode(zp, M, Cc, am), ref, f32, bound, "bn_act_fwd_p16 M=%d C=%d" % (M, Cc))


@pytest.mark.parametrize("size", ["uncapped", "capped"])
@pytest.mark.parametrize("Cc,act", [(32, RELU), (64, NONE)])
def test_add_act_twin(Cc, act, size):
    """viai_bn_add_act_fwd_twin: the fp32 z against fp64, its exact maximum, and the P16 copy decoded against the same truth"""
    L = lib()
    nt, stride = 1024, 256 * 1024
    M = 37 if size == "uncapped" else (4 * stride + 3 * nt + 5 + Cc // 4 - 1) // (Cc // 4)
    scale, shift = _coeffs("af%d" % Cc, Cc)
    res = uniform("af.res", (M, Cc), -1.0, 1.0)
    y = _off_kink(uniform("af.y", (M, Cc), -2.0, 2.0), res, scale, shift)
    gamma, beta, m_stat = scale.abs() * 2.0, shift, 2
    ref = act64(y.double() * scale.double() + shift.double() + res.double(), act)
    f32 = act64(y * scale + shift + res, act)
    z, zp = torch.full((M, Cc), float("nan"), device="cuda"), torch.full((M, Cc), float("nan"), device="cuda")
    zam, pam = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda")
    ram = dev(res.abs().max().reshape(1))
    d = [dev(t) for t in (y, scale, shift, gamma, beta)]
    rd = dev(res)
    ok(L.viai_bn_add_act_fwd_twin(*[t.data_ptr() for t in d], m_stat, rd.data_ptr(), ram.data_ptr(), z.data_ptr(), zp.data_ptr(), M, Cc, act, SLOPE,
                                  zam.data_ptr(), pam.data_ptr(), st()), "viai_bn_add_act_fwd_twin")
    what = "bn_add_act_twin M=%d C=%d" % (M, Cc)
    check_abs(z, ref, f32, what + " z")
    assert_bitwise(zam, host(z).abs().max().reshape(1), what + " z_amax")
    assert abs(float(zam) - float(ref.abs().max())) <= bound_abs(ref, f32)
    want = _fwd_bound(gamma, beta, m_stat) + float(res.abs().max())
    bound = float(pam)
    assert want <= bound <= want * 1.0011 and float(ref.abs().max()) <= bound, (bound, want)
    check_p16(_decode(zp, M, Cc, pam), ref, f32, bound, what + " z_p16")


# ---------------------------------------------------------------- pool-fused backward

def _pool_inputs(tag, N, H, W, Cc):
    """y whose values are distinct per channel and at least 4 / M apart (a hashed permutation of a grid): after BatchNorm with |gamma| >= 0.6 the
    two largest values of any window differ by more than 1e-3 (asserted by the caller)"""
    M = N * H * W
    rank = torch.argsort(torch.argsort(uniform(tag, (M, Cc)), dim=0), dim=0)
    return (-1.0 + 4.0 * rank.double() / M).float()


@pytest.mark.parametrize("addends", [1, 2])
@pytest.mark.parametrize("act", [NONE, RELU], ids=lambda a: ACT_IDS[a])
@pytest.mark.parametrize("k,s,p,N,H,W,Cc", [(3, 2, 1, 2, 8, 12, 32), (3, 2, 1, 2, 9, 11, 32), (2, 2, 0, 2, 8, 8, 24), (3, 1, 1, 1, 5, 7, 32)])
def test_pool_bwd(k, s, p, N, H, W, Cc, act, addends):
    L = lib()
    M = N * H * W
    y = _pool_inputs("pb.y", N, H, W, Cc)
    gamma = uniform("pb.g", (Cc,), 0.6, 1.4)
    beta = uniform("pb.b", (Cc,), 0.2, 0.8).clone()
    for _ in range(50):
        mean, var, _ = _stats64(y)
        invstd = 1.0 / torch.sqrt(var + BN_EPS)
        near = (((y.double() - mean) * invstd * gamma.double() + beta.double()).abs() < 4e-4).any(0)
        if not bool(near.any()):
            break
        beta[near] += 1.1e-3
    mean32, invstd32 = mean.float(), invstd.float()
    scale32 = gamma * invstd32
    shift32 = beta - mean32 * scale32
    OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    dp = [uniform("pb.dp%d" % i, (N, OH, OW, Cc), -1.0, 1.0) for i in range(addends)]

    def truth(dtype):
        yv = y.detach().to(dtype).clone().requires_grad_(True)
        g = gamma.detach().to(dtype).clone().requires_grad_(True)
        b = beta.detach().to(dtype).clone().requires_grad_(True)
        mu = yv.mean(0)
        xhat = (yv - mu) / torch.sqrt(((yv - mu) ** 2).mean(0) + BN_EPS)
        z = act64(xhat * g + b, act)
        zt = z.reshape(N, H, W, Cc).permute(0, 3, 1, 2)
        out, widx = F.max_pool2d(zt, k, s, p, return_indices=True)
        grad = dp[0].to(dtype) if addends == 1 else (dp[0] + dp[1]).to(dtype) if dtype == torch.float32 else dp[0].double() + dp[1].double()
        out.backward(grad.permute(0, 3, 1, 2))
        return yv.grad, g.grad, b.grad, zt.detach(), out.detach(), widx

    dy64, dg64, db64, z64, out64, widx = truth(torch.float64)
    dy32, dg32, db32 = truth(torch.float32)[:3]
    # the generator's properties, checked before the GPU sees anything: no pre-activation near the kink; in every window the winner leads by more
    # than 1e-3 or the whole window is the ReLU's exact zero (no gradient reaches y through it either way)
    pre = y.double() * scale32.double() + shift32.double()
    assert bool((pre.abs() > 1e-4).all())
    zz = z64.contiguous().clone()
    zz.view(N, Cc, -1).scatter_(2, widx.reshape(N, Cc, -1), float("-inf"))
    gap = out64 - F.max_pool2d(zz, k, s, p)
    assert bool(((gap > 1e-3) | (out64 == 0)).all()), "generator: a near-tie inside a window"
    iy, ix = widx // W, widx % W
    oy, ox = torch.arange(OH).view(1, 1, OH, 1), torch.arange(OW).view(1, 1, 1, OW)
    idx = ((iy - (oy * s - p)) * k + (ix - (ox * s - p))).permute(0, 2, 3, 1).contiguous().to(torch.uint8)

    nblk = L.viai_bn_bwd_blocks(M, Cc)
    part = torch.full((2 * Cc * nblk,), float("nan"), device="cuda")
    sums = torch.full((2 * Cc,), float("nan"), device="cuda")
    dg, db = torch.full((Cc,), float("nan"), device="cuda"), torch.full((Cc,), float("nan"), device="cuda")
    dy = torch.full((M, Cc), float("nan"), device="cuda")
    am = torch.zeros(1, device="cuda")
    dpd = [dev(t) for t in dp]
    idd = idx.cuda()
    d = [dev(t) for t in (y, mean32, invstd32, scale32, shift32)]
    tail = [t.data_ptr() for t in d] + [part.data_ptr(), sums.data_ptr(), dg.data_ptr(), db.data_ptr(), dy.data_ptr(), Cc, act, SLOPE, 1, am.data_ptr(), st()]
    if addends == 1:
        ok(L.viai_bn_act_pool_bwd_amax(dpd[0].data_ptr(), idd.data_ptr(), N, H, W, k, s, p, *tail), "viai_bn_act_pool_bwd_amax")
    else:
        ok(L.viai_bn_act_pool_bwd_amax2(dpd[0].data_ptr(), dpd[1].data_ptr(), idd.data_ptr(), N, H, W, k, s, p, *tail), "viai_bn_act_pool_bwd_amax2")
    what = "pool_bwd k%d s%d p%d %dx%dx%dx%d %s x%d" % (k, s, p, N, H, W, Cc, ACT_IDS[act], addends)
    check_abs(dg, dg64, dg32, what + " dgamma")
    check_abs(db, db64, db32, what + " dbeta")
    check_abs(dy, dy64, dy32, what + " dy")
    assert_bitwise(am, host(dy).abs().max().reshape(1), what + " amax")
    assert abs(float(am) - float(dy64.abs().max())) <= bound_abs(dy64, dy32)
    if act == NONE and addends == 1:
        assert L.viai_bn_act_pool_bwd_amax(dpd[0].data_ptr(), idd.data_ptr(), N, H, W, k, s, p, *(tail[:11] + [LRELU] + tail[12:])) == INVALID
