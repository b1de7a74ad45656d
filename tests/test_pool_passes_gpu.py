"""Pooling, resampling and layout passes (csrc/resample.hip, plus viai_add_act_bwd_from_output of csrc/bn.hip) called directly at the C ABI and
compared with torch on the CPU: bitwise where the pass rounds nothing, against fp64 otherwise (tests/passes_common.py: how the bounds are made).

Branch table -- one row per launch, the parametrisation that reaches each branch:

  launch                              branch                                                   reached by
  maxpool_fwd_kernel<false>           k3 s2 p1 / k2 s2 p0 / k3 s1 p1 (overlap) / k3 s3 p0      test_maxpool KSP x maps 17x22, 7x7, 2x2 x C in {4, 36}
                                      window clipped by the padding, map smaller than window   maps 2x2 (k3 p1), 7x7 edges
                                      ties: first maximum in window order, also across padding planted in every case (see _plant_ties)
                                      (3,3,0) on 2x2: torch refuses; the library's truncating    test_maxpool_window_larger_than_the_map (hand-written maximum)
                                      division gives ONE window clipped to the map
  maxpool_bwd_kernel                  oy_lo / ox_lo numerator negative (guard), k != 3, s = 1,  the same cases; fp64 autograd
                                      p = 0, up to 9 windows per pixel
  bn_act_maxpool3_fwd_kernel<false>   stem pool (3,2,1), compile-time extents, odd / even map  test_bn_act_maxpool_fwd (3,2,1) on 9x11 and 8x12
  maxpool_fwd_kernel<true>            any other window                                         test_bn_act_maxpool_fwd (2,2,0), (3,1,1)
  bn_act_maxpool3_fwd_kernel<true>    viai_bn_act_maxpool_fwd_twin (P16 copy), odd / even map  test_bn_act_maxpool_fwd (3,2,1) on 9x11x32 and 8x12x64: fp32 copy, bytes,
                                                                                               decoded P16 copy against fp64; other windows refused
  avgpool2d_fwd / _bwd_kernel         (3,2,1) on 16x16, 15x17, 3x3; (2,2,0); edge windows of   test_avgpool2d, C in {1, 5}
                                      4 and 6 taps, count_include_pad=False
  avgpool_hw_fwd / _bwd_kernel        P in {1, 49, 50}, C in {4, 512}                          test_avgpool_hw
  avgpool_h_fwd / _bwd_kernel         k = 3, IH % 3 in {0, 1, 2}; zero-filled backward rows    test_avgpool_h
  add_relu_fwd / relu_bwd /           uncapped; n4 > 8192 * 256 (grid wraps); +-0 planted;     test_join_passes n in {2052, 4 * (8192 * 256 + 777)}
  add_act_bwd_out_kernel              n % 4 != 0 refused                                       test_join_passes_refuse_ragged
  nchw_to_nhwc4_kernel                C in {1..4}, HW in {1, 255, 50176}, N in {1, 3}; amax    test_nchw_to_nhwc4
                                      with the maximum in the last pixel; C = 0, 5 refused
  act_bwd_out_kernel (bn.hip)         all four activations; n > 8192 * 256 (grid wraps)        test_act_bwd_from_output
  bilinear_fwd_px_kernel              8192-block cap reached (C = 4, 1449 x 1449 outputs)      test_bilinear_wrapped[fwd_px]
  bilinear_fwd_kernel                 C / 4 = 3, cap reached (840 x 841 outputs)               test_bilinear_wrapped[fwd_generic]
  bilinear_bwd_px_kernel<6>           cap reached (C = 4, 1449 x 1449 inputs)                  test_bilinear_wrapped[bwd_px]
  bilinear_bwd_kernel                 C / 4 = 3, cap reached (840 x 841 inputs)                test_bilinear_wrapped[bwd_generic]
  bn_act_bilinear_fwd_kernel<ACT>     256-block cap reached (C = 4, 513 x 515 outputs)         test_bn_act_bilinear_wrapped
  bn_act_bilinear_fwd_kernel<.,true>  P16 form                                                 tests/test_p16_gpu.py at the model's shapes; no wrapped case
  bilinear_*: uncapped sizes          tests/test_kernels_gpu.py::test_bilinear_ac_matches_torch_cpu holds that table.  The generic path behind
                                      npix >= 2^24 (about 270 MB per tensor) is NOT run by any test
"""
import pytest
import torch
import torch.nn.functional as F

from passes_common import (INVALID, LRELU, NONE, RELU, SIGMOID, SLOPE, act64, assert_bitwise, bound_abs, check_abs, check_p16, dev, host, lib, ok, st,
                           uniform)

pytestmark = pytest.mark.gpu

# worst error measured on the MI355X per pass family (bounds are made per case from the fp32 restatement: passes_common)
MEASURED = {       # worst (error / bound) over the cases, and that case's error
    "maxpool_bwd": "0.25 of the bound = the fp32 restatement's own error (6.0e-7 on 5.2 at k3 s1 p1 17x22 C36: nine addends)",
    "bn_act_maxpool_fwd": "0.13 of the bound: 1.2e-7 on 3.7",
    "avgpool2d fwd / bwd": "0.25 of the bound = the fp32 restatement's own error (2.4e-7 on 2.7 / 3.3e-8 on 0.45)",
    "avgpool_hw fwd / bwd": "0.28 of the bound: 4.6e-7 on 1.5 (P = 50, C = 512) / 1.3e-9 on 0.02",
    "bn_act_maxpool_fwd_twin": "fp32 copy as above; decoded P16 copy 0.21 of value bound + storage error (3.6e-7, planes bounded by 6.0)",
    "bilinear wrapped fwd / bwd": "0.13 of the bound: 6.2e-6 on 2.0 (the source index is an fp32 product, in torch's fp32 too) / 0.25: 8.4e-5 on 1.0",
    "bn_act_bilinear wrapped": "0.11 of the bound: 1.8e-6 on 2.7",
    "avgpool_h fwd / bwd": "0.40 of the bound: 3.2e-7 on 2.9 / 0.26: 2.0e-8 on 0.33",
}

KSP = [(3, 2, 1), (2, 2, 0), (3, 1, 1), (3, 3, 0)]
MAPS = [(17, 22), (7, 7), (2, 2)]


def _out_hw(IH, IW, k, s, p):
    return (IH + 2 * p - k) // s + 1, (IW + 2 * p - k) // s + 1


def _window_bytes(flat_idx, IW, OH, OW, k, s, p):
    """torch's flat argmax (iy * IW + ix; N, C, OH, OW) -> position in the window, a * k + b, as the kernels store it (N, OH, OW, C) uint8"""
    iy, ix = flat_idx // IW, flat_idx % IW
    oy = torch.arange(OH).view(1, 1, OH, 1)
    ox = torch.arange(OW).view(1, 1, 1, OW)
    b = (iy - (oy * s - p)) * k + (ix - (ox * s - p))
    assert int(b.min()) >= 0 and int(b.max()) < k * k
    return b.permute(0, 2, 3, 1).contiguous().to(torch.uint8)


def _plant_ties(x, k, s, p):
    """x (N, H, W, C): plant equal maxima inside one window -- in the first window (which the padding clips when p > 0: positions (0, 0) and
    (0, 1) are its first valid taps) and, where the map has one, in an interior window, at its first and last tap"""
    N, H, W, C = x.shape
    x = x.clone()
    if W >= 2:
        x[:, 0, 0, :] = 5.0
        x[:, 0, 1, :] = 5.0
    OH, OW = _out_hw(H, W, k, s, p)
    if OH >= 3 and OW >= 3:
        y0, x0 = 1 * s - p, 2 * s - p
        x[:, y0, x0, 0::2] = 6.0
        x[:, y0 + k - 1, x0 + k - 1, 0::2] = 6.0
    return x


# every (k, s, p) on every map, except the one pool that does not exist: (3, 3, 0) on 2 x 2 (see the branch table)
MAXPOOL_CASES = [(k, s, p, H, W) for (k, s, p) in KSP for (H, W) in MAPS if H + 2 * p >= k]
assert len(MAXPOOL_CASES) == 11


@pytest.mark.parametrize("Cc", [4, 36])
@pytest.mark.parametrize("k,s,p,H,W", MAXPOOL_CASES)
def test_maxpool(k, s, p, H, W, Cc):
    L = lib()
    N = 2
    x = _plant_ties(uniform("mp.x", (N, H, W, Cc), -2.0, 2.0), k, s, p)
    OH, OW = _out_hw(H, W, k, s, p)
    xt = x.permute(0, 3, 1, 2)
    want, widx = F.max_pool2d(xt, k, s, p, return_indices=True)
    xd = dev(x)
    y = torch.full((N, OH, OW, Cc), float("nan"), device="cuda")
    idx = torch.full((N, OH, OW, Cc), 255, dtype=torch.uint8, device="cuda")
    ok(L.viai_maxpool_fwd(xd.data_ptr(), y.data_ptr(), idx.data_ptr(), N, H, W, Cc, k, s, p, st()), "viai_maxpool_fwd")
    assert_bitwise(y, want.permute(0, 2, 3, 1).contiguous(), "maxpool values")
    wb = _window_bytes(widx, W, OH, OW, k, s, p)
    assert_bitwise(idx, wb, "maxpool argmax bytes")
    # backward: fp64 autograd of the same pool
    dy = uniform("mp.dy", (N, OH, OW, Cc))
    x64 = xt.double().requires_grad_(True)
    F.max_pool2d(x64, k, s, p).backward(dy.permute(0, 3, 1, 2).double())
    x32 = xt.clone().requires_grad_(True)
    F.max_pool2d(x32, k, s, p).backward(dy.permute(0, 3, 1, 2))
    dx = torch.full((N, H, W, Cc), float("nan"), device="cuda")
    dyd, ib = dev(dy), wb.cuda()
    ok(L.viai_maxpool_bwd(dyd.data_ptr(), ib.data_ptr(), dx.data_ptr(), N, H, W, Cc, k, s, p, st()), "viai_maxpool_bwd")
    check_abs(dx, x64.grad.permute(0, 2, 3, 1), x32.grad.permute(0, 2, 3, 1), "maxpool_bwd k%d s%d p%d %dx%d C%d" % (k, s, p, H, W, Cc))


def _distinct_map(tag, shape):
    """(N, H, W, C) with all values of a channel distinct and at least 4 / M apart (a hashed permutation of a grid over [-1, 3))"""
    N, H, W, Cc = shape
    M = N * H * W
    rank = torch.argsort(torch.argsort(uniform(tag, (M, Cc)), dim=0), dim=0)
    return (-1.0 + 4.0 * rank.double() / M).float().reshape(shape)


@pytest.mark.parametrize("act", [NONE, RELU], ids=["none", "relu"])
@pytest.mark.parametrize("k,s,p,H,W,Cc", [(3, 2, 1, 9, 11, 32), (3, 2, 1, 8, 12, 24), (3, 2, 1, 8, 12, 64), (2, 2, 0, 8, 8, 24), (3, 1, 1, 5, 7, 32)])
def test_bn_act_maxpool_fwd(k, s, p, H, W, Cc, act):
    L = lib()
    N = 2
    y = _distinct_map("bmp.y", (N, H, W, Cc))
    scale = uniform("bmp.sc", (Cc,), 0.6, 1.4)
    shift = uniform("bmp.sh", (Cc,), -0.9, -0.3).clone()
    for _ in range(50):                 # move a channel's shift until none of its pre-activations lies near the activation's kink
        near = ((y.double() * scale.double() + shift.double()).abs() < 2e-4).reshape(-1, Cc).any(0)
        if not bool(near.any()):
            break
        shift[near] += 7e-4
    pre = y.double() * scale.double() + shift.double()
    assert bool((pre.abs() > 1e-4).all()), "generator: a pre-activation within 1e-4 of the kink"
    z64 = act64(pre, act)
    OH, OW = _out_hw(H, W, k, s, p)
    want, widx = F.max_pool2d(z64.permute(0, 3, 1, 2), k, s, p, return_indices=True)
    # the generator's property: the winner of every window leads the runner-up by more than 1e-3, or the whole window is the ReLU's exact 0
    # (then the first tap wins, in torch and in the kernel alike)
    neg = F.max_pool2d(z64.permute(0, 3, 1, 2), k, s, p)
    zz = z64.permute(0, 3, 1, 2).contiguous()
    zz.view(N, Cc, -1).scatter_(2, widx.reshape(N, Cc, -1), float("-inf"))
    gap = neg - F.max_pool2d(zz, k, s, p)
    assert bool(((gap > 1e-3) | (neg == 0)).all()), "generator: a near-tie inside a window"
    z32 = act64(y * scale + shift, act)
    f32 = F.max_pool2d(z32.permute(0, 3, 1, 2), k, s, p)
    yd, sd, hd = dev(y), dev(scale), dev(shift)
    out = torch.full((N, OH, OW, Cc), float("nan"), device="cuda")
    idx = torch.full((N, OH, OW, Cc), 255, dtype=torch.uint8, device="cuda")
    am = torch.zeros(1, device="cuda")
    ok(L.viai_bn_act_maxpool_fwd(yd.data_ptr(), sd.data_ptr(), hd.data_ptr(), out.data_ptr(), idx.data_ptr(), N, H, W, Cc, k, s, p, act, SLOPE,
                                 am.data_ptr(), st()), "viai_bn_act_maxpool_fwd")
    check_abs(out, want.permute(0, 2, 3, 1), f32.permute(0, 2, 3, 1), "bn_act_maxpool_fwd k%d s%d p%d %dx%d act%d" % (k, s, p, H, W, act))
    assert_bitwise(idx, _window_bytes(widx, W, OH, OW, k, s, p), "bn_act_maxpool argmax bytes")
    assert_bitwise(am, host(out).abs().max().reshape(1), "bn_act_maxpool amax")
    assert abs(float(am) - float(want.abs().max())) <= bound_abs(want, f32)
    if (k, s, p) == (3, 2, 1) and Cc % 32 == 0:
        # the twin: the same fp32 tensor and bytes, plus a P16 copy whose scale comes from |gamma| sqrt(m_stat - 1) + |beta| (here gamma = 2 |scale|,
        # beta = shift, m_stat = 5: |scale y + shift| <= 4 |scale| + |shift| on y in [-1, 3))
        gamma, beta, m_stat = scale.abs() * 2.0, shift, 5
        out2 = torch.full((N, OH, OW, Cc), float("nan"), device="cuda")
        outp = torch.full((N, OH, OW, Cc), float("nan"), device="cuda")
        idx2 = torch.full((N, OH, OW, Cc), 255, dtype=torch.uint8, device="cuda")
        am2, pam = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda")
        gd, bd = dev(gamma), dev(beta)
        ok(L.viai_bn_act_maxpool_fwd_twin(yd.data_ptr(), sd.data_ptr(), hd.data_ptr(), gd.data_ptr(), bd.data_ptr(), m_stat, out2.data_ptr(), outp.data_ptr(),
                                          idx2.data_ptr(), N, H, W, Cc, k, s, p, act, SLOPE, am2.data_ptr(), pam.data_ptr(), st()), "viai_bn_act_maxpool_fwd_twin")
        check_abs(out2, want.permute(0, 2, 3, 1), f32.permute(0, 2, 3, 1), "bn_act_maxpool_fwd_twin %dx%dx%d act%d" % (H, W, Cc, act))
        assert_bitwise(idx2, _window_bytes(widx, W, OH, OW, k, s, p), "twin argmax bytes")
        assert_bitwise(am2, host(out2).abs().max().reshape(1), "twin amax")
        bnd = float((gamma.double().abs() * 2.0 + beta.double().abs()).max())
        assert bnd <= float(pam) <= bnd * 1.0011 and float(want.abs().max()) <= float(pam), (float(pam), bnd)
        dec = torch.full((N, OH, OW, Cc), float("nan"), device="cuda")
        ok(L.viai_p16_decode(outp.data_ptr(), dec.data_ptr(), N * OH * OW, Cc, pam.data_ptr(), st()), "viai_p16_decode")
        check_p16(dec, want.permute(0, 2, 3, 1), f32.permute(0, 2, 3, 1), float(pam), "bn_act_maxpool_fwd_twin P16 %dx%dx%d act%d" % (H, W, Cc, act))
        assert L.viai_bn_act_maxpool_fwd_twin(yd.data_ptr(), sd.data_ptr(), hd.data_ptr(), gd.data_ptr(), bd.data_ptr(), m_stat, out2.data_ptr(), outp.data_ptr(),
                                              idx2.data_ptr(), N, H, W, Cc, 2, 2, 0, act, SLOPE, am2.data_ptr(), pam.data_ptr(), st()) == INVALID
    assert L.viai_bn_act_maxpool_fwd(yd.data_ptr(), sd.data_ptr(), hd.data_ptr(), out.data_ptr(), idx.data_ptr(), N, H, W, Cc, k, s, p, 3, SLOPE,
                                     am.data_ptr(), st()) == INVALID                      # sigmoid: refused


@pytest.mark.parametrize("Cc", [1, 5])
@pytest.mark.parametrize("k,s,p,H,W", [(3, 2, 1, 16, 16), (3, 2, 1, 15, 17), (3, 2, 1, 3, 3), (2, 2, 0, 16, 16), (2, 2, 0, 15, 17)])
def test_avgpool2d(k, s, p, H, W, Cc):
    L = lib()
    N = 2
    x = uniform("ap.x", (N, H, W, Cc), -1.0, 3.0)
    OH, OW = _out_hw(H, W, k, s, p)
    dy = uniform("ap.dy", (N, OH, OW, Cc))
    xt = x.permute(0, 3, 1, 2)
    x64 = xt.double().requires_grad_(True)
    y64 = F.avg_pool2d(x64, k, s, p, count_include_pad=False)
    y64.backward(dy.permute(0, 3, 1, 2).double())
    x32 = xt.clone().requires_grad_(True)
    y32 = F.avg_pool2d(x32, k, s, p, count_include_pad=False)
    y32.backward(dy.permute(0, 3, 1, 2))
    xd, dyd = dev(x), dev(dy)
    y = torch.full((N, OH, OW, Cc), float("nan"), device="cuda")
    dx = torch.full((N, H, W, Cc), float("nan"), device="cuda")
    ok(L.viai_avgpool2d_fwd(xd.data_ptr(), y.data_ptr(), N, H, W, Cc, k, s, p, st()), "viai_avgpool2d_fwd")
    ok(L.viai_avgpool2d_bwd(dyd.data_ptr(), dx.data_ptr(), N, H, W, Cc, k, s, p, st()), "viai_avgpool2d_bwd")
    check_abs(y, y64.detach().permute(0, 2, 3, 1), y32.detach().permute(0, 2, 3, 1), "avgpool2d_fwd k%d %dx%d C%d" % (k, H, W, Cc))
    check_abs(dx, x64.grad.permute(0, 2, 3, 1), x32.grad.permute(0, 2, 3, 1), "avgpool2d_bwd k%d %dx%d C%d" % (k, H, W, Cc))


@pytest.mark.parametrize("Cc", [4, 512])
@pytest.mark.parametrize("P", [1, 49, 50])
def test_avgpool_hw(P, Cc):
    L = lib()
    N = 3
    x = uniform("ahw.x", (N, P, Cc), -1.0, 3.0)
    dy = uniform("ahw.dy", (N, Cc))
    xd, dyd = dev(x), dev(dy)
    y = torch.full((N, Cc), float("nan"), device="cuda")
    dx = torch.full((N, P, Cc), float("nan"), device="cuda")
    ok(L.viai_avgpool_hw_fwd(xd.data_ptr(), y.data_ptr(), N, P, Cc, st()), "viai_avgpool_hw_fwd")
    ok(L.viai_avgpool_hw_bwd(dyd.data_ptr(), dx.data_ptr(), N, P, Cc, st()), "viai_avgpool_hw_bwd")
    seq = torch.zeros(N, Cc)
    for q in range(P):                  # the plain fp32 formula: one accumulator per output, pixels in order
        seq = seq + x[:, q, :]
    check_abs(y, x.double().mean(1), seq / P, "avgpool_hw_fwd P%d C%d" % (P, Cc))
    check_abs(dx, (dy.double() / P)[:, None, :].expand(N, P, Cc), (dy / P)[:, None, :].expand(N, P, Cc), "avgpool_hw_bwd P%d C%d" % (P, Cc))


@pytest.mark.parametrize("IH", [6, 7, 8])
def test_avgpool_h(IH):
    L = lib()
    N, Wd, Cc, k = 2, 5, 12, 3
    OH = IH // k
    x = uniform("ah.x", (N, IH, Wd, Cc), -1.0, 3.0)
    dy = uniform("ah.dy", (N, OH, Wd, Cc))
    x64 = x.double().permute(0, 3, 1, 2).requires_grad_(True)
    y64 = F.avg_pool2d(x64, (k, 1))
    y64.backward(dy.double().permute(0, 3, 1, 2))
    x32 = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    y32 = F.avg_pool2d(x32, (k, 1))
    y32.backward(dy.permute(0, 3, 1, 2))
    xd, dyd = dev(x), dev(dy)
    y = torch.full((N, OH, Wd, Cc), float("nan"), device="cuda")
    dx = torch.full((N, IH, Wd, Cc), float("nan"), device="cuda")
    ok(L.viai_avgpool_h_fwd(xd.data_ptr(), y.data_ptr(), N, IH, Wd, Cc, k, st()), "viai_avgpool_h_fwd")
    ok(L.viai_avgpool_h_bwd(dyd.data_ptr(), dx.data_ptr(), N, IH, Wd, Cc, k, st()), "viai_avgpool_h_bwd")
    check_abs(y, y64.detach().permute(0, 2, 3, 1), y32.detach().permute(0, 2, 3, 1), "avgpool_h_fwd IH%d" % IH)
    check_abs(dx, x64.grad.permute(0, 2, 3, 1), x32.grad.permute(0, 2, 3, 1), "avgpool_h_bwd IH%d" % IH)
    assert bool((host(dx)[:, OH * k:] == 0).all())                       # rows past the last whole window: exactly zero
    assert L.viai_avgpool_h_fwd(xd.data_ptr(), y.data_ptr(), N, 2, Wd, Cc, k, st()) == INVALID          # no whole window
    assert L.viai_avgpool_h_fwd(xd.data_ptr(), y.data_ptr(), N, IH, Wd, 6, k, st()) == INVALID          # C % 4


@pytest.mark.parametrize("n", [2052, 4 * (8192 * 256 + 777)])
def test_join_passes(n):
    """relu(a + b), its backward from the output, and the two-addend backward: bit for bit, with +0, -0 and exact cancellations planted"""
    L = lib()
    draw = uniform("jn.draw", (4 * (8192 * 256 + 777) + 3,))            # one draw, four shifted views of it
    a, b = draw[0:n].clone(), draw[1:n + 1].clone()
    a[0::7] = -b[0::7]                  # a + b = +0
    a[1::11], b[1::11] = -0.0, -0.0     # a + b = -0
    a[2::13], b[2::13] = 0.0, 0.0
    g, g2 = draw[2:n + 2], draw[3:n + 3]
    zero = torch.zeros(())
    s = a + b
    want = torch.where(s > 0, s, zero)
    ad, bd, gd, g2d = dev(a), dev(b), dev(g), dev(g2)
    out = torch.full((n,), float("nan"), device="cuda")
    ok(L.viai_add_relu_fwd(ad.data_ptr(), bd.data_ptr(), out.data_ptr(), n, st()), "viai_add_relu_fwd")
    assert_bitwise(out, want, "add_relu")
    d = torch.full((n,), float("nan"), device="cuda")
    ok(L.viai_relu_bwd(gd.data_ptr(), out.data_ptr(), d.data_ptr(), n, st()), "viai_relu_bwd")
    assert_bitwise(d, torch.where(want > 0, g, zero), "relu_bwd")
    d2 = torch.full((n,), float("nan"), device="cuda")
    ok(L.viai_add_act_bwd_from_output(gd.data_ptr(), g2d.data_ptr(), out.data_ptr(), d2.data_ptr(), n, RELU, SLOPE, st()), "viai_add_act_bwd_from_output")
    assert_bitwise(d2, (g + g2) * (want > 0).float(), "add_act_bwd_from_output relu")             # a product: the masked elements keep the sum's sign (-0)
    if n == 2052:
        ok(L.viai_add_act_bwd_from_output(gd.data_ptr(), g2d.data_ptr(), out.data_ptr(), d2.data_ptr(), n, 2, SLOPE, st()), "viai_add_act_bwd_from_output")
        slope32 = torch.tensor(SLOPE, dtype=torch.float32)
        assert_bitwise(d2, (g + g2) * torch.where(want > 0, torch.ones(()), slope32), "add_act_bwd_from_output lrelu")


def test_join_passes_refuse_ragged():
    L = lib()
    t = torch.zeros(16, device="cuda")
    for n in (1, 6, 15):
        assert L.viai_add_relu_fwd(t.data_ptr(), t.data_ptr(), t.data_ptr(), n, st()) == INVALID
        assert L.viai_relu_bwd(t.data_ptr(), t.data_ptr(), t.data_ptr(), n, st()) == INVALID
        assert L.viai_add_act_bwd_from_output(t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), n, RELU, SLOPE, st()) == INVALID


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("HW", [1, 255, 50176])
@pytest.mark.parametrize("Cc", [1, 2, 3, 4])
def test_nchw_to_nhwc4(Cc, HW, N):
    L = lib()
    x = uniform("lay.x", (N, Cc, HW), -3.0, 3.0).clone()
    x[N - 1, Cc - 1, HW - 1] = -8.5                          # the maximum, in the last pixel's last channel
    want = torch.zeros(N, HW, 4)
    want[:, :, :Cc] = x.permute(0, 2, 1)
    xd = dev(x)
    for with_amax in (False, True):
        y = torch.full((N, HW, 4), float("nan"), device="cuda")
        am = torch.zeros(1, device="cuda")
        if with_amax:
            ok(L.viai_nchw_to_nhwc4_amax(xd.data_ptr(), y.data_ptr(), N, Cc, HW, am.data_ptr(), st()), "viai_nchw_to_nhwc4_amax")
            assert float(am) == 8.5
        else:
            ok(L.viai_nchw_to_nhwc4(xd.data_ptr(), y.data_ptr(), N, Cc, HW, st()), "viai_nchw_to_nhwc4")
        assert_bitwise(y, want, "nchw_to_nhwc4 C%d" % Cc)              # padded channels: +0 bit for bit
    for bad in (0, 5):
        assert L.viai_nchw_to_nhwc4(xd.data_ptr(), y.data_ptr(), N, bad, HW, st()) == INVALID
    assert L.viai_nchw_to_nhwc4_amax(xd.data_ptr(), y.data_ptr(), N, Cc, HW, 0, st()) == INVALID


def test_maxpool_window_larger_than_the_map():
    """(3, 3, 0) on a 2 x 2 map: nn.MaxPool2d has no output here; the library's output extent (2 - 3) / 3 + 1 truncates to 1, so it computes ONE window
    clipped to the map.  Pinned against a hand-written maximum over the four pixels (first maximum in row-major order, byte = iy * 3 + ix)."""
    L = lib()
    N, H, W, Cc, k, s, p = 2, 2, 2, 8, 3, 3, 0
    x = uniform("mp.small", (N, H, W, Cc), -2.0, 2.0).clone()
    x[0, 0, 1, 0] = x[0, 1, 0, 0] = 3.0                        # a tie: the first in row-major order wins
    flat = x.reshape(N, H * W, Cc)
    want, pos = flat.max(1)
    first = (flat == want[:, None, :]).float().argmax(1)           # first index holding the maximum
    byte = ((first // W) * k + first % W).to(torch.uint8)
    xd = dev(x)
    y = torch.full((N, 1, 1, Cc), float("nan"), device="cuda")
    idx = torch.full((N, 1, 1, Cc), 255, dtype=torch.uint8, device="cuda")
    ok(L.viai_maxpool_fwd(xd.data_ptr(), y.data_ptr(), idx.data_ptr(), N, H, W, Cc, k, s, p, st()), "viai_maxpool_fwd")
    assert_bitwise(y.reshape(N, Cc), want, "maxpool 3x3 window on a 2x2 map")
    assert_bitwise(idx.reshape(N, Cc), byte, "its argmax bytes")
    dy = uniform("mp.small.dy", (N, 1, 1, Cc))
    dx = torch.full((N, H, W, Cc), float("nan"), device="cuda")
    dyd = dev(dy)
    ok(L.viai_maxpool_bwd(dyd.data_ptr(), idx.data_ptr(), dx.data_ptr(), N, H, W, Cc, k, s, p, st()), "viai_maxpool_bwd")
    wantdx = torch.zeros(N, H * W, Cc).scatter_(1, first[:, None, :], dy.reshape(N, 1, Cc)).reshape(N, H, W, Cc)
    assert_bitwise(dx, wantdx, "its backward")


@pytest.mark.parametrize("n", [1027, 8192 * 256 + 777])
@pytest.mark.parametrize("act", [NONE, RELU, LRELU, SIGMOID], ids=["none", "relu", "lrelu", "sigmoid"])
def test_act_bwd_from_output(act, n):
    """dx = dz * act'(.) from the activation's OUTPUT z: two fp32 products at the most, bit for bit"""
    L = lib()
    draw = uniform("jn.draw", (4 * (8192 * 256 + 777) + 3,))
    g = draw[5:n + 5]
    z = draw[9:n + 9].clone()
    if act == SIGMOID:
        z = z * 0.5 + 0.5
    z[0::9] = 0.0
    z[1::9] = -0.0
    one = torch.ones(())
    if act == SIGMOID:
        d = z * (one - z)
    elif act == RELU:
        d = (z > 0).float()
    elif act == LRELU:
        d = torch.where(z > 0, one, torch.tensor(SLOPE, dtype=torch.float32))
    else:
        d = torch.ones_like(z)
    gd, zd = dev(g), dev(z)
    dx = torch.full((n,), float("nan"), device="cuda")
    ok(L.viai_act_bwd_from_output(gd.data_ptr(), zd.data_ptr(), dx.data_ptr(), n, act, SLOPE, st()), "viai_act_bwd_from_output")
    assert_bitwise(dx, g * d, "act_bwd_from_output act%d n=%d" % (act, n))


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("which", ["fwd_px", "fwd_generic", "bwd_px", "bwd_generic"])
def test_bilinear_wrapped(which):
    """F.interpolate(mode="bilinear", align_corners=True) where the 8192-block cap of the streaming grid is reached (more than 8192 * 256 channel quads):
    the per-pixel kernels at C = 4, the generic ones at C = 12 (C / 4 no power of two)"""
    L = lib()
    Cc, big = (4, (1449, 1449)) if which.endswith("px") else (12, (840, 841))
    small = (37, 41)
    assert big[0] * big[1] * (Cc // 4) > 8192 * 256
    if which.startswith("fwd"):
        (IH, IW), (OH, OW) = small, big
        x = uniform("bl.x", (1, IH, IW, Cc), -2.0, 2.0)
        xt = x.permute(0, 3, 1, 2)
        ref = _nhwc(F.interpolate(xt.double(), size=[OH, OW], mode="bilinear", align_corners=True))
        f32 = _nhwc(F.interpolate(xt, size=[OH, OW], mode="bilinear", align_corners=True))
        xd = dev(x)
        y = torch.full((1, OH, OW, Cc), float("nan"), device="cuda")
        ok(L.viai_bilinear_ac_fwd(xd.data_ptr(), y.data_ptr(), 1, IH, IW, OH, OW, Cc, st()), "viai_bilinear_ac_fwd")
        check_abs(y, ref, f32, "bilinear %s" % which)
    else:
        (IH, IW), (OH, OW) = big, small
        dy = uniform("bl.dy", (1, OH, OW, Cc), -1.0, 1.0)
        outs = []
        for dtype in (torch.float64, torch.float32):
            xin = torch.zeros(1, Cc, IH, IW, dtype=dtype, requires_grad=True)
            F.interpolate(xin, size=[OH, OW], mode="bilinear", align_corners=True).backward(dy.permute(0, 3, 1, 2).to(dtype))
            outs.append(_nhwc(xin.grad))
        dyd = dev(dy)
        dx = torch.full((1, IH, IW, Cc), float("nan"), device="cuda")
        ok(L.viai_bilinear_ac_bwd(dyd.data_ptr(), dx.data_ptr(), 1, IH, IW, OH, OW, Cc, st()), "viai_bilinear_ac_bwd")
        check_abs(dx, outs[0], outs[1], "bilinear %s" % which)


def test_bn_act_bilinear_wrapped():
    """out = interpolate(relu(scale y + shift)) with more output pixels (513 x 515) than the 256 blocks of 1024 pixels hold at C = 4"""
    L = lib()
    Cc, IH, IW, OH, OW = 4, 20, 23, 513, 515
    assert OH * OW > 256 * 1024
    scale, shift = uniform("bl.sc", (Cc,), 0.6, 1.4), uniform("bl.sh", (Cc,), -0.5, 0.5)
    y = uniform("bl.y", (1, IH, IW, Cc), -2.0, 2.0)
    near = (y.double() * scale.double() + shift.double()).abs() < 2e-4
    y = torch.where(near, y + 1e-3, y)
    pre = y.double() * scale.double() + shift.double()
    assert bool((pre.abs() > 1e-4).all())
    z64, z32 = act64(pre, RELU), act64(y * scale + shift, RELU)
    ref = _nhwc(F.interpolate(z64.permute(0, 3, 1, 2), size=[OH, OW], mode="bilinear", align_corners=True))
    f32 = _nhwc(F.interpolate(z32.permute(0, 3, 1, 2), size=[OH, OW], mode="bilinear", align_corners=True))
    yd, sd, hd = dev(y), dev(scale), dev(shift)
    out = torch.full((1, OH, OW, Cc), float("nan"), device="cuda")
    am = torch.zeros(1, device="cuda")
    ok(L.viai_bn_act_bilinear_fwd_amax(yd.data_ptr(), sd.data_ptr(), hd.data_ptr(), out.data_ptr(), 1, IH, IW, OH, OW, Cc, RELU, SLOPE, am.data_ptr(), st()),
       "viai_bn_act_bilinear_fwd_amax")
    check_abs(out, ref, f32, "bn_act_bilinear wrapped")
    assert abs(float(am) - float(z64.abs().max())) <= bound_abs(z64, z32)              # every input pixel is a tap of the up-sampling: max |z| of the map
