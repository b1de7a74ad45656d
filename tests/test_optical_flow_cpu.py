"""CPU: the optical-flow rule (include/viai_hip.h) without a device.  The host mirror `tvl1_host` (plain C++ over the same
per-pixel functions the kernels call) against the independent fp64 numpy restatement of the header's text; identical frames give exactly zero
flow, bytes of 128 and an empty motion box; a known sub-pixel shift is recovered; the encoding is exact; and every entry point refuses bad
arguments before it does anything, so also here.

Measured on the CPU (seed-0 texture, scales=3, warps=2, iterations=7, shift (0.8, -0.6)): max |host - fp64| = 5.4e-6 at 35 x 51 and 8.6e-6 at
70 x 131 (other seeds: up to 1.9e-5); asserted at four times the measured value.  Known motion (64 x 96, shift (1.5, -0.75), scales=3, default
warps and iterations): the fp64 restatement's mean interior end-point error is 0.0093 px, the host mirror's 0.0093 px; asserted at twice the
restatement's."""
import ctypes as C
import os

import numpy as np
import pytest

import optical_flow_common as F

INVALID = 1                                                               # hipErrorInvalidValue
MEASURED_DIFF = {(35, 51): 5.4e-6, (70, 131): 8.6e-6}                     # max |host mirror - fp64 restatement|, measured (docstring)
MEASURED_EPE_FP64 = 0.0093                                                # mean interior end-point error of the fp64 restatement, px
SHIFT = (1.5, -0.75)


@pytest.fixture(scope="module")
def lib():
    from viai_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


# ----------------------------------------------------------------------------- 1. the host mirror is the rule
@pytest.mark.parametrize("H,W", sorted(MEASURED_DIFF))
def test_host_mirror_equals_the_fp64_restatement(H, W, lib):
    from viai_amd.optical_flow import tvl1_host
    assert F.level_shapes(H, W, 3) == ([(35, 51), (18, 26)] if H == 35 else [(70, 131), (35, 66), (18, 33)])
    assert lib.viai_optical_flow_levels(H, W, 3) == len(F.level_shapes(H, W, 3))
    frames = F.texture(3, H, W, (0.8, -0.6), seed=0)
    got, want = tvl1_host(frames, **F.QUICK), F.tvl1_rule(frames, **F.QUICK)
    assert got.dtype == np.float32 and got.shape == (2, 2, H, W)
    diff = float(np.abs(got - want).max())
    print("max |host - fp64| at %d x %d: %.3e (max |flow| %.3f)" % (H, W, diff, np.abs(want).max()))
    assert np.abs(want).max() > 0.5                                       # there is a flow to be wrong about
    assert diff <= 4 * MEASURED_DIFF[(H, W)], diff


def test_host_mirror_reads_colour_as_the_rule_says(lib):
    from viai_amd.optical_flow import tvl1_host
    rgb = F.rgb_of(F.texture(2, 35, 51, (0.8, -0.6), seed=0))
    for bgr in (False, True):
        diff = float(np.abs(tvl1_host(rgb, bgr=bgr, **F.QUICK) - F.tvl1_rule(rgb, bgr=bgr, **F.QUICK)).max())
        assert diff <= 4 * MEASURED_DIFF[(35, 51)], (bgr, diff)
    assert np.array_equal(tvl1_host(rgb, bgr=True, **F.QUICK), tvl1_host(np.ascontiguousarray(rgb[..., ::-1]), **F.QUICK))
    assert not np.array_equal(tvl1_host(rgb, bgr=True, **F.QUICK), tvl1_host(rgb, **F.QUICK))
    grey = F.grey_rule(rgb).astype(np.uint8)                              # (N, H, W) is taken as grey, and so is C = 1
    assert np.array_equal(tvl1_host(grey, **F.QUICK), tvl1_host(rgb, **F.QUICK))
    assert np.array_equal(tvl1_host(grey[..., None], **F.QUICK), tvl1_host(grey, **F.QUICK))


def test_the_host_result_does_not_depend_on_iters_per_launch(lib):
    from viai_amd.optical_flow import tvl1_host
    frames = F.texture(2, 35, 51, (0.8, -0.6), seed=1)
    assert np.array_equal(tvl1_host(frames, iters_per_launch=1, **F.QUICK), tvl1_host(frames, iters_per_launch=8, **F.QUICK))


# ----------------------------------------------------------------------------- 2. identical frames
def test_identical_frames_are_still(lib):
    from viai_amd.optical_flow import encode_u8_host, tvl1_host
    from viai_amd.video import motion_box_host
    frames = np.repeat(F.texture(1, 70, 131, (0, 0), seed=2), 4, axis=0)
    flow = tvl1_host(frames, **F.QUICK)
    assert flow.shape == (3, 2, 70, 131) and np.all(flow == 0.0)          # every term is exactly zero
    fx, fy = encode_u8_host(flow)
    assert fx.shape == fy.shape == (4, 70, 131) and np.all(fx == 128) and np.all(fy == 128)
    # |128 - 127| + |128 - 127| per frame is exactly the reference's threshold 2 N, which is strict: nothing moves
    assert motion_box_host(fx, fy).tolist() == [0, 0, 0, 0, 0]
    assert np.all(F.tvl1_rule(frames, **F.QUICK) == 0.0)


# ----------------------------------------------------------------------------- 3. a known motion
def test_a_known_shift_is_recovered(lib):
    from viai_amd.optical_flow import tvl1_host
    frames = F.texture(2, 64, 96, SHIFT, seed=0)
    kw = dict(F.DEFAULTS, scales=3)
    epe64 = F.epe_interior(F.tvl1_rule(frames, **kw)[0], SHIFT)
    epe = F.epe_interior(tvl1_host(frames, **kw)[0].astype(np.float64), SHIFT)
    print("mean interior end-point error: fp64 restatement %.4f px, host mirror %.4f px" % (epe64, epe))
    assert abs(epe64 - MEASURED_EPE_FP64) < 5e-4, epe64                   # the recorded figure is the restatement's
    assert epe <= 2 * MEASURED_EPE_FP64, epe
    assert epe < 0.5 * float(np.hypot(*SHIFT))                            # a zero flow can never pass


# ----------------------------------------------------------------------------- 4. the encoding
def test_encoding_is_exact(lib):
    from viai_amd.optical_flow import encode_u8_host
    r = np.random.RandomState(3)
    flow = (r.randn(3, 2, 9, 13) * 12).astype(np.float32)
    edge = np.array([0.0, -0.0, 20.0, -20.0, 20.000002, -20.000002, 25.0, -1e9, 1e9, np.inf, -np.inf, 19.96, -19.96, 0.0784, 0.0785],
                    dtype=np.float32)
    flow[0, 0, 0, :] = edge[:13]
    flow[0, 1, 0, :2] = edge[13:]
    for pad in (True, False):
        fx, fy = encode_u8_host(flow, pad_last=pad)
        wx, wy = F.encode_rule(flow, pad_last=pad)
        assert fx.dtype == np.uint8 and fx.shape == (3 + pad, 9, 13)
        assert np.array_equal(fx, wx) and np.array_equal(fy, wy)
    fx, fy = encode_u8_host(flow)
    assert fx[0, 0, :11].tolist() == [128, 128, 255, 0, 255, 0, 255, 0, 255, 255, 0]
    assert np.array_equal(fx[3], fx[2]) and np.array_equal(fy[3], fy[2])  # pad_last repeats the last map
    # exact ties: with bound 127.5 the code is rint(f + 127.5), so an integer f is a tie, and ties go to the even code
    ties = np.zeros((1, 2, 1, 6), dtype=np.float32)
    ties[0, 0, 0] = [0, 1, 2, 3, -1, -2]
    tx, _ = encode_u8_host(ties, bound=127.5, pad_last=False)
    assert tx[0, 0].tolist() == [128, 128, 130, 130, 126, 126]
    assert np.array_equal(tx, F.encode_rule(ties, 127.5, False)[0])
    for bound in (5.0, 32.0):
        assert np.array_equal(encode_u8_host(flow, bound=bound)[1], F.encode_rule(flow, bound)[1])


# ----------------------------------------------------------------------------- 5. refusals
def test_host_entry_points_refuse_bad_arguments(lib):
    H, W = 20, 24
    frames = np.zeros((3, H, W, 3), dtype=np.uint8)
    flow = np.zeros((2, 2, H, W), dtype=np.float32)
    pf, po = frames.ctypes.data_as(C.c_void_p), flow.ctypes.data_as(C.c_void_p)
    nan = float("nan")

    def call(frames=pf, stride=H * W * 3, N=3, H=H, W=W, Cn=3, tau=0.25, lam=0.15, theta=0.3, scales=3, warps=1, iterations=2, ipl=4, flow=po):
        return lib.viai_optical_flow_host(frames, stride, N, H, W, Cn, 0, tau, lam, theta, scales, warps, iterations, ipl, flow)

    assert call() == 0
    bad = [dict(frames=None), dict(flow=None), dict(N=1), dict(N=0), dict(H=0), dict(W=0), dict(H=1 << 15), dict(W=1 << 15),
           dict(stride=H * W * 3 - 1), dict(Cn=2), dict(scales=0), dict(warps=0), dict(iterations=0), dict(ipl=0), dict(ipl=9)]
    for name in ("tau", "lam", "theta"):
        bad += [{name: 0.0}, {name: -1.0}, {name: nan}]
    for kw in bad:
        assert call(**kw) == INVALID, kw
    assert np.all(flow == 0.0)                                            # zero frames give zero flow, and a refused call writes nothing

    fx, fy = np.zeros((3, H, W), dtype=np.uint8), np.zeros((3, H, W), dtype=np.uint8)
    px, py = fx.ctypes.data_as(C.c_void_p), fy.ctypes.data_as(C.c_void_p)

    def enc(flow=po, pairs=2, H=H, W=W, bound=20.0, fx=px, fy=py):
        return lib.viai_flow_encode_u8_host(flow, pairs, H, W, bound, 1, fx, fy)

    assert enc() == 0
    for kw in (dict(flow=None), dict(fx=None), dict(fy=None), dict(pairs=0), dict(H=0), dict(W=0), dict(H=1 << 15), dict(W=1 << 15),
               dict(bound=0.0), dict(bound=-20.0), dict(bound=nan)):
        assert enc(**kw) == INVALID, kw
    assert lib.viai_optical_flow_ws_bytes(0, H, W, 3) == 0 and lib.viai_optical_flow_ws_bytes(2, 1 << 15, W, 3) == 0
    assert lib.viai_optical_flow_ws_bytes(2, H, W, 3) == 4 * (3 * H * W + 16 * 2 * H * W)       # one level: the short side is below 32
    assert lib.viai_optical_flow_launches(480, 640, 5, 5, 30, 1) == 1 + 4 + 25 * 31 + 4 + 1
    assert lib.viai_optical_flow_launches(480, 640, 5, 5, 30, 8) == 1 + 4 + 25 * 5 + 4 + 1
    assert lib.viai_optical_flow_launches(480, 640, 5, 5, 30, 9) == 0


def test_the_wrappers_validate_and_the_device_ones_refuse_the_cpu(lib):
    import torch

    from viai_amd import _lib, optical_flow as O
    frames = np.zeros((3, 20, 24), dtype=np.uint8)
    for kw in (dict(scales=0), dict(iterations=0), dict(iters_per_launch=9), dict(tau=0.0), dict(theta=float("nan")), dict(lam=-1.0)):
        with pytest.raises(ValueError):
            O.tvl1_host(frames, **kw)
    with pytest.raises(TypeError):
        O.tvl1_host(frames, epsilon=0.01)                                 # there is no epsilon stop
    with pytest.raises(ValueError):
        O.tvl1_host(frames[:1])
    with pytest.raises(ValueError):
        O.encode_u8_host(np.zeros((1, 2, 4, 4), dtype=np.float32), bound=0.0)
    with pytest.raises(_lib.ViaiLibraryError):
        O.tvl1(torch.zeros(3, 20, 24, dtype=torch.uint8))
    with pytest.raises(_lib.ViaiLibraryError):
        O.encode_u8(torch.zeros(1, 2, 4, 4))
    with pytest.raises(_lib.ViaiLibraryError):
        O.flow_u8(torch.zeros(3, 20, 24, 3, dtype=torch.uint8))
    import viai_amd
    assert viai_amd.tvl1 is O.tvl1 and viai_amd.flow_u8 is O.flow_u8 and viai_amd.encode_u8_host is O.encode_u8_host
