"""Losses, the Adam step and the small reductions (csrc/loss_opt.hip, viai_absmax in csrc/bn.hip, viai_colsum in csrc/conv_direct.hip) called
directly at the C ABI and compared with an fp64 restatement on the CPU (tests/passes_common.py: how the bounds are made).

Branch table -- one row per launch, the parametrisation that reaches each branch:

  launch                           branch                                              reached by
  loss_part_kernel<BCE|MSE|L1>     one block, fewer elements than threads              test_loss_fwd n = 1, 255
                                   two blocks (n > 4096)                               test_loss_fwd n = 4097
                                   65 blocks, 16 elements per thread                   test_loss_fwd n = 262145
                                   block cap (1024) reached, grid-stride wraps         test_loss_fwd n = 4096 * 1024 + 4097
  loss_final_kernel                nb < 256 / nb = 1024 (4 partials per thread)        the same n; 1024 partials at the last
  loss_part_kernel<BCE>            log clamp at -100                                   test_bce_edges p in {0, 1}
  loss_bwd_kernel<BCE|MSE|L1>      uncapped / capped at 4096 blocks (wraps)            test_loss_bwd: the same n (the last wraps 4x) 
                                   gscale NULL / device scalar                         test_loss_bwd gs in {None, 3.0}
                                   BCE denominator floor 1e-12                         test_bce_edges p in {0, 1, 1e-30}
                                   L1 subgradient at a == b                            test_l1_subgradient_at_equal_inputs_is_zero
  adam_tick_kernel + adam_kernel   1 block / 2 blocks / 4096 blocks wrapped            test_adam n = 1, 257, 4096 * 256 + 513; grad_scale 1, 1/16
  absmax_kernel                    no quad at all (n < 4), tail of n % 4 in block 0    test_absmax n = 1, 2, 3; 5, 1023, 262147
                                   quads only                                          test_absmax n = 4
                                   more than one block                                 test_absmax n = 262147 (257 blocks)
                                   running max (seeded above / below)                  test_absmax seed in {0, small, large}
                                   misaligned pointer refused                          test_absmax_refusals
  colsum_part / colsum_final       one row, one quad                                   test_colsum (1, 4)
                                   C/4 = 6 does not divide 256 (idle lanes)            test_colsum (1000, 24)
                                   547 blocks of 128 rows, short last block (113)      test_colsum (70001, 32)
                                   accumulate 0 / 1                                    test_colsum acc
                                   C % 4 != 0 (scalar path)                            covered by tests/test_kernels_gpu.py (conv bias gradients, Cout = 1)
  range_count_kernel               over / max / non-finite, inf and NaN                test_range_count
  axpy_kernel, mask_mul_kernel     4096-block cap reached, grid wraps                  test_axpy_and_mask_mul_wrapped
  step_scalars_kernel              with / without contrast; out[5] untouched           test_step_scalars

Worst errors measured on the MI355X: MEASURED below.
"""
import math

import numpy as np
import pytest
import torch

from passes_common import INVALID, assert_bitwise, check_abs, check_rel, dev, host, lib, ok, ptr, st, uniform

pytestmark = pytest.mark.gpu

# worst error measured on the MI355X per pass family (the bounds themselves are made per case from the fp32 restatement: passes_common)
MEASURED = {       # worst (error / bound) over the cases, and that case's error
    "bce / mse / l1 fwd": "0.37 of the bound: 8.4e-8 abs at bce n = 255 (bound 2.3e-7: the 2-ulp floor)",
    "bce / mse / l1 bwd": "0.25 of the bound = the fp32 restatement's own error (1.0e-7 .. 1.1e-7 relative)",
    "adam p, m, v": "0.25 of the bound (v at n = 257, step 2: 1.3e-5 relative on gradients of 1e-9, as the fp32 restatement)",
    "colsum": "0.28 of the bound: 3.0e-5 abs on sums of 287 at (1000, 24)",
    "axpy": "0.18 of the bound: 6.0e-8",
    "step_scalars": "0.15 of the bound: 4.8e-7 on 13.0",
}

LOSS_N = [1, 255, 4097, 262145, 4096 * 1024 + 4097]


def _prob(tag, n):
    return uniform(tag, (n,), 0.02, 0.98)


def _loss64(kind, a, b_or_t):
    a = a.double()
    if kind == "bce":
        t = b_or_t
        return -(t * torch.log(a).clamp_min(-100.0) + (1.0 - t) * torch.log(1.0 - a).clamp_min(-100.0))
    if kind == "mse":
        return (a - b_or_t) ** 2
    return (a - b_or_t.double()).abs()


def _loss32(kind, a, b_or_t):
    if kind == "bce":
        t = b_or_t
        return -(t * torch.log(a).clamp_min(-100.0) + (1.0 - t) * torch.log(1.0 - a).clamp_min(-100.0))
    if kind == "mse":
        return (a - b_or_t) ** 2
    return (a - b_or_t).abs()


def _run_fwd(kind, a, b_or_t):
    L = lib()
    n = a.numel()
    nb = L.viai_reduce_blocks(n)
    assert nb == min(1024, max(1, (n + 4095) // 4096))
    part = torch.full((nb,), float("nan"), device="cuda")
    loss = torch.full((1,), float("nan"), device="cuda")
    ad = dev(a)
    if kind == "l1":
        bd = dev(b_or_t)
        ok(L.viai_l1_fwd(ad.data_ptr(), bd.data_ptr(), n, part.data_ptr(), loss.data_ptr(), st()), "viai_l1_fwd")
    else:
        fn = L.viai_bce_fwd if kind == "bce" else L.viai_mse_fwd
        ok(fn(ad.data_ptr(), float(b_or_t), n, part.data_ptr(), loss.data_ptr(), st()), "viai_%s_fwd" % kind)
    return host(loss)


@pytest.mark.parametrize("n", LOSS_N)
@pytest.mark.parametrize("kind,t", [("bce", 1.0), ("bce", 0.0), ("mse", 1.0), ("l1", None)])
def test_loss_fwd(kind, t, n):
    a = _prob("loss.a", n)
    b = _prob("loss.b", n) if kind == "l1" else t
    ref = _loss64(kind, a, b).sum().reshape(1) / n
    f32 = (_loss32(kind, a, b).sum() / n).reshape(1)
    check_abs(_run_fwd(kind, a, b), ref, f32, "%s_fwd n=%d" % (kind, n))


def _grad64(kind, x, t, gs, n):
    x = x.double()
    t = t.double() if torch.is_tensor(t) else t
    if kind == "bce":
        g = (x - t) / ((1.0 - x) * x).clamp_min(1e-12)
    elif kind == "mse":
        g = 2.0 * (x - t)
    else:
        g = torch.sign(x - t)
    return g * (gs / n)


def _grad32(kind, x, t, gs, n):
    if kind == "bce":
        g = (x - t) / ((1.0 - x) * x).clamp_min(1e-12)
    elif kind == "mse":
        g = 2.0 * (x - t)
    else:
        g = torch.sign(x - t)
    return g * (torch.tensor(gs, dtype=torch.float32) / torch.tensor(float(n), dtype=torch.float32))


def _run_bwd(kind, a, b_or_t, gs):
    L = lib()
    n = a.numel()
    ad = dev(a)
    da = torch.full((n,), float("nan"), device="cuda")
    gsd = None if gs is None else torch.tensor([gs], device="cuda")
    if kind == "l1":
        bd = dev(b_or_t)
        ok(L.viai_l1_bwd(ad.data_ptr(), bd.data_ptr(), n, ptr(gsd), da.data_ptr(), st()), "viai_l1_bwd")
    else:
        fn = L.viai_bce_bwd if kind == "bce" else L.viai_mse_bwd
        ok(fn(ad.data_ptr(), float(b_or_t), n, ptr(gsd), da.data_ptr(), st()), "viai_%s_bwd" % kind)
    return host(da)


@pytest.mark.parametrize("n", LOSS_N)
@pytest.mark.parametrize("gs", [None, 3.0])
@pytest.mark.parametrize("kind,t", [("bce", 1.0), ("bce", 0.0), ("mse", 1.0), ("l1", None)])
def test_loss_bwd(kind, t, gs, n):
    a = _prob("loss.a", n)
    b = _prob("loss.b", n) if kind == "l1" else t
    g = 1.0 if gs is None else gs
    got = _run_bwd(kind, a, b, gs)
    check_rel(got, _grad64(kind, a, b, g, n), _grad32(kind, a, b, g, n), "%s_bwd n=%d gs=%s" % (kind, n, gs))


@pytest.mark.parametrize("t", [1.0, 0.0])
def test_bce_edges(t):
    """the log clamp at p in {0, 1} (an element costs exactly 100 or 0) and the gradient's denominator floor at p in {0, 1, 1e-30}"""
    n = 259
    a = _prob("loss.edge", n).clone()
    a[0], a[1], a[2], a[n - 1], a[n - 2] = 0.0, 1.0, 1e-30, 0.0, 1.0
    ref = _loss64("bce", a, t).sum().reshape(1) / n
    assert float(_loss64("bce", a, t)[0]) in (0.0, 100.0) and float(_loss64("bce", a, t)[1]) in (0.0, 100.0)
    check_abs(_run_fwd("bce", a, t), ref, (_loss32("bce", a, t).sum() / n).reshape(1), "bce_fwd edges t=%g" % t)
    got = _run_bwd("bce", a, t, None)
    want = _grad64("bce", a, t, 1.0, n)
    assert math.isfinite(float(got.abs().max()))
    # p = 0, t = 0 gives an exact 0 / 1e-12 = 0: compare those absolutely, the rest relatively
    nz = want != 0
    assert bool((got[~nz] == 0).all())
    check_rel(got[nz], want[nz], _grad32("bce", a, t, 1.0, n)[nz], "bce_bwd edges t=%g" % t)
    assert abs(float(got[2]) - (1e-30 - t) / 1e-12 / n) <= 4 * 2.0 ** -23 * abs((1e-30 - t) / 1e-12 / n)


def test_l1_subgradient_at_equal_inputs_is_zero():
    n = 4097
    a = _prob("loss.a", n)
    b = _prob("loss.b", n).clone()
    b[::3] = a[::3]
    got = _run_bwd("l1", a, b, 3.0)
    assert bool((got[::3] == 0).all()) and bool((got[::3].view(torch.int32) == 0).all())
    want = _grad32("l1", a, b, 3.0, n)
    check_rel(got[want != 0], _grad64("l1", a, b, 3.0, n)[want != 0], want[want != 0], "l1_bwd ties")
    assert float(_run_fwd("l1", a, a.clone())) == 0.0


def test_loss_refuses_empty():
    L = lib()
    z = torch.zeros(4, device="cuda")
    assert L.viai_bce_fwd(z.data_ptr(), 1.0, 0, z.data_ptr(), z.data_ptr(), st()) == INVALID
    assert L.viai_l1_bwd(z.data_ptr(), z.data_ptr(), 0, 0, z.data_ptr(), st()) == INVALID
    assert L.viai_adam_step(z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), 0, z.data_ptr(), 0.9, 0.999, 1e-8, 1.0, st()) == INVALID


# ---------------------------------------------------------------- Adam

def _adam_sim(dtype, p, g, steps, lr, b1, b2, eps, gscale):
    """torch.optim.Adam (no amsgrad, no weight decay) restated; dtype fp64 is the truth, fp32 the scale (tests/passes_common.py).  In fp32 every
    constant is rounded to fp32 first (a Python float times an fp32 tensor is an fp32 product)"""
    r = (lambda x: x) if dtype == torch.float64 else (lambda x: float(np.float32(x)))
    p = p.to(dtype).clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    out = []
    for t in range(1, steps + 1):
        gi = g[t - 1].to(dtype) * r(gscale)
        m = m * r(b1) + gi * r(1.0 - r(b1))
        v = v * r(b2) + gi * gi * r(1.0 - r(b2))
        bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
        p = p - (m / (v.sqrt() / r(math.sqrt(bc2)) + r(eps))) * r(lr / bc1)
        out.append((p.clone(), m.clone(), v.clone()))
    return out


@pytest.mark.parametrize("n", [1, 257, 4096 * 256 + 513])
@pytest.mark.parametrize("gscale", [1.0, 1.0 / 16])
def test_adam(n, gscale):
    L = lib()
    lr, b1, b2, eps, steps = 1e-3, 0.9, 0.999, 1e-8, 3
    p0 = uniform("adam.p", (n,), -1.0, 1.0)
    # gradients spanning 1e-9 .. 1 in magnitude, both signs
    g = [torch.sign(uniform("adam.s%d" % t, (n,))) * (10.0 ** (-9.0 * uniform("adam.e%d" % t, (n,), 0.0, 1.0).double())).float() for t in range(steps)]
    ref = _adam_sim(torch.float64, p0, g, steps, lr, b1, b2, eps, gscale)
    f32 = _adam_sim(torch.float32, p0, g, steps, lr, b1, b2, eps, gscale)
    p, m, v = dev(p0), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    state = torch.tensor([0.0, lr, 1.0, 1.0], dtype=torch.float64, device="cuda")
    pw1, pw2 = 1.0, 1.0
    for t in range(steps):
        gd = dev(g[t])
        ok(L.viai_adam_step(p.data_ptr(), gd.data_ptr(), m.data_ptr(), v.data_ptr(), n, state.data_ptr(), b1, b2, eps, gscale, st()), "viai_adam_step")
        pw1, pw2 = pw1 * b1, pw2 * b2
        assert host(state).tolist() == [float(t + 1), lr, pw1, pw2]          # the same fp64 products: exact
        check_abs(p, ref[t][0], f32[t][0], "adam p n=%d step %d" % (n, t + 1))
        check_rel(m, ref[t][1], f32[t][1], "adam m n=%d step %d" % (n, t + 1))
        check_rel(v, ref[t][2], f32[t][2], "adam v n=%d step %d" % (n, t + 1))


# ---------------------------------------------------------------- abs-max

@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 1023, 262147])
def test_absmax(n):
    L = lib()
    base = uniform("absmax.x", (n,), -1.0, 1.0)
    spots = sorted(set([0, min(3, n - 1), max(0, (n // 4) * 4 - 1), max(0, (n // 4) * 4 - 4)] + list(range((n // 4) * 4, n))))
    for spot in spots:
        for val in (7.25, -9.5):
            x = base.clone()
            x[spot] = val
            xd = dev(x)
            for seed in (0.0, 0.5, 100.0):
                am = torch.tensor([seed], device="cuda")
                ok(L.viai_absmax(xd.data_ptr(), n, am.data_ptr(), st()), "viai_absmax")
                assert float(am) == max(seed, abs(val)), (n, spot, val, seed, float(am))
    # and the plain maximum of the draw, bit for bit
    am = torch.zeros(1, device="cuda")
    xd = dev(base)
    ok(L.viai_absmax(xd.data_ptr(), n, am.data_ptr(), st()), "viai_absmax")
    assert_bitwise(am, base.abs().max().reshape(1), "absmax n=%d" % n)


def test_absmax_refusals():
    L = lib()
    x = torch.ones(64, device="cuda")
    am = torch.zeros(1, device="cuda")
    assert x.data_ptr() % 16 == 0
    assert L.viai_absmax(x.data_ptr() + 4, 8, am.data_ptr(), st()) == INVALID          # misaligned for the 16-byte loads
    assert L.viai_absmax(0, 8, am.data_ptr(), st()) == INVALID
    assert L.viai_absmax(x.data_ptr(), 8, 0, st()) == INVALID
    assert L.viai_absmax(x.data_ptr(), -1, am.data_ptr(), st()) == INVALID
    ok(L.viai_absmax(x.data_ptr(), 0, am.data_ptr(), st()), "viai_absmax n=0")
    assert float(am) == 0.0


# ---------------------------------------------------------------- column sums, counts, axpy, mask, scalars

@pytest.mark.parametrize("M,Cc", [(1, 4), (1000, 24), (70001, 32)])
@pytest.mark.parametrize("acc", [0, 1])
def test_colsum(M, Cc, acc):
    L = lib()
    x = uniform("colsum.x", (M, Cc), -1.0, 1.0) + 0.25
    nb = L.viai_colsum_blocks(M, Cc)
    rows = max((M + 2047) // 2048, max(4, 4096 // Cc))
    assert nb == (M + rows - 1) // rows
    if M == 70001:
        assert nb == 547 and M - (nb - 1) * rows == 113             # 128-row blocks, a short last one
    part = torch.full((nb * Cc,), float("nan"), device="cuda")
    out0 = uniform("colsum.o", (Cc,), -5.0, 5.0)
    out = dev(out0)
    xd = dev(x)
    ok(L.viai_colsum(xd.data_ptr(), M, Cc, part.data_ptr(), out.data_ptr(), acc, st()), "viai_colsum")
    ref = x.double().sum(0) + (out0.double() if acc else 0.0)
    f32 = x.sum(0) + (out0 if acc else 0.0)
    check_abs(out, ref, f32, "colsum (%d, %d) acc=%d" % (M, Cc, acc))


def test_range_count():
    L = lib()
    n = 300001
    x = uniform("range.x", (n,), -4.0, 4.0).clone()
    x[5], x[n - 1], x[77777] = float("inf"), float("-inf"), float("nan")
    x[123456] = -1234.5
    limit = 3.0
    xn = x.numpy()
    fin = np.isfinite(xn)
    counts = torch.tensor([10, 0, 20], dtype=torch.int32, device="cuda")
    xd = dev(x)
    ok(L.viai_range_count(xd.data_ptr(), n, limit, counts.data_ptr(), st()), "viai_range_count")
    got = host(counts).tolist()
    assert got[0] == 10 + int((np.abs(xn[fin]) > limit).sum())
    assert got[1] == int(np.array([1234.5], dtype=np.float32).view(np.int32)[0])
    assert got[2] == 20 + 3
    ok(L.viai_range_count(xd.data_ptr(), 0, limit, counts.data_ptr(), st()), "viai_range_count n=0")
    assert host(counts).tolist() == got


def test_axpy_and_mask_mul_wrapped():
    L = lib()
    N, F, T = 3, 517, 677                   # 1 050 027 elements > 4096 * 256: the grid wraps; F, T odd
    n = N * F * T
    assert n > 4096 * 256
    s = uniform("mm.s", (N, F, T))
    mask = (uniform("mm.m", (N, T)) > 0).float()
    out = torch.full((N, F, T), float("nan"), device="cuda")
    sd, md = dev(s), dev(mask)
    ok(L.viai_mask_mul(sd.data_ptr(), md.data_ptr(), out.data_ptr(), N, F, T, st()), "viai_mask_mul")
    assert_bitwise(out, s * mask[:, None, :], "mask_mul")
    x, y0, a = uniform("axpy.x", (n,)), uniform("axpy.y", (n,)), -0.37
    y = dev(y0)
    xd = dev(x)
    ok(L.viai_axpy(a, xd.data_ptr(), y.data_ptr(), n, st()), "viai_axpy")
    a32 = float(np.float32(a))
    check_abs(y, y0.double() + a32 * x.double(), y0 + np.float32(a) * x, "axpy wrapped")


@pytest.mark.parametrize("with_contrast", [False, True])
def test_step_scalars(with_contrast):
    L = lib()
    vals = [0.6931, 0.7123, 0.65, 0.1234, 2.5]          # d_real, d_fake, g_gan, l1, contrast
    dv = [torch.tensor([v], device="cuda") for v in vals]
    out = torch.full((6,), -77.0, device="cuda")
    l1w, cw = 100.0, 0.5
    ok(L.viai_step_scalars(dv[0].data_ptr(), dv[1].data_ptr(), dv[2].data_ptr(), dv[3].data_ptr(), dv[4].data_ptr() if with_contrast else 0,
                           l1w, cw, out.data_ptr(), st()), "viai_step_scalars")
    v64 = [float(np.float32(v)) for v in vals]
    ref = [0.5 * (v64[1] + v64[0]), v64[2] + l1w * v64[3] + (cw * v64[4] if with_contrast else 0.0), v64[2], v64[3], v64[0]]
    v32 = [np.float32(v) for v in vals]
    lg = v32[2] + np.float32(l1w) * v32[3]
    if with_contrast:
        lg = lg + np.float32(cw) * v32[4]
    f32 = [np.float32(0.5) * (v32[1] + v32[0]), lg, v32[2], v32[3], v32[0]]
    got = host(out)
    check_abs(got[:5], torch.tensor(ref, dtype=torch.float64), torch.tensor([float(v) for v in f32], dtype=torch.float32), "step_scalars")
    assert float(got[5]) == (v64[4] if with_contrast else -77.0)
    assert L.viai_step_scalars(0, dv[1].data_ptr(), dv[2].data_ptr(), dv[3].data_ptr(), 0, l1w, cw, out.data_ptr(), st()) == INVALID
