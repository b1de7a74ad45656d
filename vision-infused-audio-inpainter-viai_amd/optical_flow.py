"""Optical flow on the device (csrc/optical_flow.hip): raw uint8 frames in, TV-L1 flow and the dataset's 8-bit flow maps out,
so that `VideoFrontEnd(image)` alone gives the blocks of the generator's visual branch.

    tvl1            frames (N, H, W, 3) or (N, H, W) uint8 on the GPU -> flow (N - 1, 2, H, W) fp32, pixels per frame, map i = frame i -> i + 1
    encode_u8       flow -> (flow_x, flow_y) uint8, `round(255 (f + bound) / (2 bound))`, a still pixel is 128
    flow_u8         the two together: what `VideoFrontEnd` and `motion_box` take
    tvl1_host       the same rule on numpy arrays, in plain C++ on the host (`viai_optical_flow_host`): no GPU needed
    encode_u8_host  likewise

The rule is stated in full in include/viai_hip.h; its per-pixel arithmetic is written once (csrc/viai_flow_rule.h) for the kernels and the host
mirror, so `tvl1` and `tvl1_host` give the same bits, and the result does not depend on `iters_per_launch`, `pairs_per_pass` or how the stack is
laid out.  That the reference's maps are TV-L1 flow in this encoding is an inference from its motion threshold, not a record, and no trained
weights are at hand: how the generator takes these maps is not tested.  Parity with OpenCV's TV-L1 is not claimed either.
"""
from __future__ import annotations

import torch

from . import _lib

ITERS_PER_LAUNCH = 8            # VIAI_FLOW_ITERS_PER_LAUNCH of include/viai_hip.h
PARAMS = dict(tau=0.25, lam=0.15, theta=0.3, scales=5, warps=5, iterations=30)


def _params(kw, what):
    p = dict(PARAMS)
    ipl = kw.pop("iters_per_launch", ITERS_PER_LAUNCH)
    for k in list(kw):
        if k not in p:
            raise TypeError("%s: unknown parameter %r" % (what, k))
        p[k] = kw.pop(k)
    for k in ("scales", "warps", "iterations"):
        if int(p[k]) != p[k] or p[k] < 1:
            raise ValueError("%s: %s is an integer >= 1" % (what, k))
    if int(ipl) != ipl or not 1 <= ipl <= 8:
        raise ValueError("%s: iters_per_launch is an integer in 1..8" % what)
    for k in ("tau", "lam", "theta"):
        if not float(p[k]) > 0:
            raise ValueError("%s: %s is positive" % (what, k))
    return (float(p["tau"]), float(p["lam"]), float(p["theta"]), int(p["scales"]), int(p["warps"]), int(p["iterations"]), int(ipl))


def _shape(shape, what):
    if len(shape) not in (3, 4) or (len(shape) == 4 and shape[3] not in (1, 3, 4)):
        raise ValueError("%s: frames are (N, H, W, 3) (or 1 or 4 channels), or grey (N, H, W)" % what)
    N, H, W = (int(v) for v in shape[:3])
    C = int(shape[3]) if len(shape) == 4 else 1
    if N < 2:
        raise ValueError("%s: at least two frames" % what)
    if not (1 <= H < 1 << 15 and 1 <= W < 1 << 15):
        raise ValueError("%s: 1 <= H, W < 2^15" % what)
    return N, H, W, C


def tvl1(frames, bgr=False, pairs_per_pass=32, **params):
    """TV-L1 flow of every pair of consecutive frames: (N - 1, 2, H, W) fp32 on the device.  frames: uint8 on the GPU, (N, H, W, C) with C = 3
    (or 4; `bgr` swaps R and B) or grey (N, H, W); the first dimension may be a view (every other frame, a range).  The stack is processed
    `pairs_per_pass` pairs at a time, which bounds the workspace (`viai_optical_flow_ws_bytes`) and changes no bit.  params: tau, lam, theta,
    scales, warps, iterations, iters_per_launch."""
    from .video import _frames_view, _need_cuda
    f = _need_cuda(frames, "tvl1")
    N, H, W, C = _shape(tuple(f.shape), "tvl1")
    args = _params(dict(params), "tvl1")
    if int(pairs_per_pass) != pairs_per_pass or not 1 <= pairs_per_pass <= 65535:
        raise ValueError("tvl1: pairs_per_pass is an integer in 1..65535")
    f, stride = _frames_view(f, H * W * C)
    lib = _lib.load()
    from .ops import _stream
    P = min(int(pairs_per_pass), N - 1)
    ws = torch.empty((int(lib.viai_optical_flow_ws_bytes(P, H, W, args[3])) + 7) // 8, dtype=torch.int64, device=f.device)
    flow = torch.empty((N - 1, 2, H, W), dtype=torch.float32, device=f.device)
    for i in range(0, N - 1, P):
        n = min(P, N - 1 - i)
        _lib.check(lib.viai_optical_flow(f[i].data_ptr(), stride, n + 1, H, W, C, int(bool(bgr)), *args, flow[i].data_ptr(), ws.data_ptr(),
                                         _stream()), "viai_optical_flow")
    return flow


def encode_u8(flow, bound=20.0, pad_last=True):
    """flow (P, 2, H, W) fp32 on the GPU -> (flow_x, flow_y), uint8 (P + pad_last, H, W): the `dense_flow` encoding, a still pixel is 128.
    pad_last repeats the last map, so that N frames give N maps."""
    if not isinstance(flow, torch.Tensor):
        raise TypeError("encode_u8: a torch tensor expected, got %s" % type(flow).__name__)
    if not flow.is_cuda:
        raise _lib.ViaiLibraryError("encode_u8 runs on the GPU only (got a %s tensor); no CPU fallback" % flow.device)
    if flow.dtype != torch.float32 or flow.dim() != 4 or flow.size(1) != 2 or flow.numel() == 0:
        raise ValueError("encode_u8: flow is fp32 (P, 2, H, W)")
    if not float(bound) > 0:
        raise ValueError("encode_u8: bound is positive")
    flow = flow.contiguous()
    P, _, H, W = flow.shape
    n = P + (1 if pad_last else 0)
    fx = torch.empty((n, H, W), dtype=torch.uint8, device=flow.device)
    fy = torch.empty((n, H, W), dtype=torch.uint8, device=flow.device)
    from .ops import _stream
    _lib.check(_lib.load().viai_flow_encode_u8(flow.data_ptr(), P, H, W, float(bound), int(bool(pad_last)), fx.data_ptr(), fy.data_ptr(),
                                               _stream()), "viai_flow_encode_u8")
    return fx, fy


def flow_u8(frames, bgr=False, bound=20.0, pad_last=True, pairs_per_pass=32, **params):
    """`encode_u8(tvl1(frames, ...), bound, pad_last)`: the two uint8 stacks the video front end takes."""
    return encode_u8(tvl1(frames, bgr=bgr, pairs_per_pass=pairs_per_pass, **params), bound, pad_last)


def tvl1_host(frames, bgr=False, **params):
    """`tvl1` on the host: a uint8 numpy array in, an fp32 numpy array (N - 1, 2, H, W) out.  Needs the built library, not a GPU."""
    import ctypes as C_

    import numpy as np
    a = np.ascontiguousarray(frames)
    if a.dtype != np.uint8:
        raise TypeError("tvl1_host: uint8 expected, got %s" % a.dtype)
    N, H, W, C = _shape(a.shape, "tvl1_host")
    args = _params(dict(params), "tvl1_host")
    flow = np.empty((N - 1, 2, H, W), dtype=np.float32)
    _lib.check(_lib.load().viai_optical_flow_host(a.ctypes.data_as(C_.c_void_p), H * W * C, N, H, W, C, int(bool(bgr)), *args,
                                                  flow.ctypes.data_as(C_.c_void_p)), "viai_optical_flow_host")
    return flow


def encode_u8_host(flow, bound=20.0, pad_last=True):
    """`encode_u8` on the host: fp32 numpy (P, 2, H, W) -> two uint8 numpy arrays."""
    import ctypes as C_

    import numpy as np
    a = np.ascontiguousarray(flow, dtype=np.float32)
    if a.ndim != 4 or a.shape[1] != 2 or a.size == 0:
        raise ValueError("encode_u8_host: flow is fp32 (P, 2, H, W)")
    if not float(bound) > 0:
        raise ValueError("encode_u8_host: bound is positive")
    P, _, H, W = a.shape
    n = P + (1 if pad_last else 0)
    fx, fy = np.empty((n, H, W), dtype=np.uint8), np.empty((n, H, W), dtype=np.uint8)
    _lib.check(_lib.load().viai_flow_encode_u8_host(a.ctypes.data_as(C_.c_void_p), P, H, W, float(bound), int(bool(pad_last)),
                                                    fx.ctypes.data_as(C_.c_void_p), fy.ctypes.data_as(C_.c_void_p)), "viai_flow_encode_u8_host")
    return fx, fy
