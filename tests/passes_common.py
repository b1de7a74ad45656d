"""Shared helpers of the direct tests of the non-conv passes (test_bn_passes_gpu.py, test_pool_passes_gpu.py, test_loss_opt_passes_gpu.py,
test_contrastive_pipeline_passes_gpu.py; contrastive_common.py draws its inputs from uniform() here).

Every test there calls one C-ABI entry point (include/viai_hip.h) on inputs from the oracle's counter-based generators and compares with a plain
fp64 restatement on the CPU.  Two kinds of assertion:

  * bitwise   -- passes that round nothing beyond their inputs (max-pool values and argmax bytes, add_relu, relu_bwd, layout, mask_mul, every
                 amax, every count);
  * measured  -- everything else: the SAME formula is evaluated in fp32 with torch on the CPU on the same inputs, its worst error against fp64
                 at that shape is the scale, and the kernel may err by MARGIN (4: another summation order, fma contraction) times that scale,
                 but the bound never falls below 2 ulp (fp32) of the output's magnitude.  The kernel's own output is never the yardstick.
"""
import functools
import math

import numpy as np
import torch

from oracle import viai_oracle as O

EPS32 = 2.0 ** -23
MARGIN = 4.0
INVALID = 1             # hipErrorInvalidValue
NONE, RELU, LRELU, SIGMOID = 0, 1, 2, 3
ACT_IDS = {NONE: "none", RELU: "relu", LRELU: "lrelu", SIGMOID: "sigmoid"}
SLOPE = 0.2


def lib():
    from viai_amd import _lib
    return _lib.load()


def st():
    return torch.cuda.current_stream().cuda_stream


def ok(err, what):
    assert err == 0, "%s returned hipError_t %d" % (what, err)


def dev(t):
    return t.detach().to(torch.float32).contiguous().cuda()


def ptr(t):
    return 0 if t is None else t.data_ptr()


def host(t):
    return t.detach().cpu()


@functools.lru_cache(maxsize=6)
def _pool(tag, size):
    return O.cf_uniform(tag, (size,), -1.0, 1.0)


def uniform(tag, shape, lo=-1.0, hi=1.0):
    """cf_uniform(tag) of the shape, scaled into [lo, hi).  A draw is a hash of (tag, flat index), so a shorter draw is a prefix of a longer one:
    the raw draw is made at the next power of two and sliced, which lets the large cases (whose sizes all differ) share one cached draw per tag;
    the cache keeps six draws at the most"""
    n = int(np.prod(shape))
    size = 1 << max(n - 1, 1).bit_length()
    u = _pool(tag, size)[:n]
    return (u * ((hi - lo) / 2.0) + ((hi + lo) / 2.0)).to(torch.float32).reshape(shape)


def act64(v, act, slope=SLOPE):
    if act == RELU:
        return torch.where(v > 0, v, torch.zeros_like(v))
    if act == LRELU:
        return torch.where(v > 0, v, v * slope)
    if act == SIGMOID:
        return torch.sigmoid(v)
    return v


def assert_bitwise(got, want, what):
    g, w = host(got).contiguous(), host(want).contiguous()
    assert g.shape == w.shape and g.dtype == w.dtype, (what, g.shape, w.shape, g.dtype, w.dtype)
    if g.dtype == torch.float32:
        g, w = g.view(torch.int32), w.view(torch.int32)
    bad = g != w
    assert not bool(bad.any()), "%s: %d of %d elements differ bit for bit, first at flat index %d" % (
        what, int(bad.sum()), bad.numel(), int(bad.reshape(-1).nonzero()[0]))


def bound_abs(ref64, f32):
    """MARGIN x the fp32 restatement's worst error, floored at 2 ulp of the tensor's magnitude"""
    scale = float((f32.double() - ref64).abs().max())
    return max(MARGIN * scale, 2.0 * EPS32 * float(ref64.abs().max()))


def check_abs(got, ref64, f32, what):
    """max |got - ref64| over the tensor against bound_abs; prints the figure before it asserts"""
    err = float((host(got).double() - ref64).abs().max())
    b = bound_abs(ref64, f32)
    print("%-40s err %.3e  bound %.3e  (fp32 restatement %.3e, |ref| %.3e)" % (
        what, err, b, float((f32.double() - ref64).abs().max()), float(ref64.abs().max())))
    assert err <= b, (what, err, b)
    return err


def check_rel(got, ref64, f32, what):
    """element by element, for passes whose outputs span many decades: |got - ref| <= max(MARGIN x worst RELATIVE fp32 error, 2 ulp) |ref|"""
    mag = ref64.abs().clamp_min(1e-300)
    scale = float(((f32.double() - ref64).abs() / mag).max())
    rel = max(MARGIN * scale, 2.0 * EPS32)
    err = (host(got).double() - ref64).abs()
    worst = float((err / mag).max())
    print("%-40s rel err %.3e  bound %.3e  (fp32 restatement %.3e)" % (what, worst, rel, scale))
    assert bool((err <= rel * ref64.abs()).all()), (what, worst, rel)
    return worst


def p16_storage_tol(ref64, bound):
    """What storing a value as two fp16 terms of value * S may cost (include/viai_hip.h, the P16 layout): S = 2^(14 - e) for a bound < 2^e; the
    leading term keeps 11 bits, the remainder 11 more of what is left (22 bits: 2^-22 relative), or -- once the remainder is subnormal in fp16 --
    one fp16 subnormal step, 2^-24 / S, absolute; the decode adds the two terms and multiplies by 1 / S in fp32 (2 x 2^-24 relative).  From the published bound alone."""
    e = math.floor(math.log2(bound)) + 1
    S = 2.0 ** (14 - e)
    return ref64.abs() * (2.0 ** -22 + 2.0 ** -23) + 2.0 ** -24 / S


def check_p16(decoded, ref64, f32, bound, what):
    """a decoded P16 tensor against the fp64 truth: the value bound of the fp32 pass (bound_abs) plus the storage error, element by element"""
    err = (host(decoded).double() - ref64).abs()
    tol = bound_abs(ref64, f32) + p16_storage_tol(ref64, bound)
    worst = float((err / tol).max())
    print("%-40s P16 worst err / bound %.3f  (max err %.3e, bound of the planes %.4g)" % (what, worst, float(err.max()), bound))
    assert bool((err <= tol).all()), (what, worst)
    return worst
