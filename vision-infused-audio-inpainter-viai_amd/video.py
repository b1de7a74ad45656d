"""Video front end on the device (csrc/video_prep.hip): raw uint8 frames and flow maps of any H x W in, the blocks the
generator's visual branch consumes out.  The counterpart of `MelFrontEnd` for the other modality.

    motion_box        the reference's motion bounding box (`crop_image` + `find_cluster`) from the two flow stacks -> int32 (5,) on the device
    motion_box_host   the same rule on numpy arrays, in plain C++ on the host (`viai_motion_box_host`): no GPU needed
    resize_u8         crop to the box, pad to a square with grey 127, resize to R x R -> uint8 (n, R, R, C)
    resize_u8_host    the same on numpy arrays (`viai_video_resize_u8_host`)
    prepare           crop + pad + resize + flip + crop + normalise in one resampling launch -> fp32 NHWC4 or (n, C, size, size)
    VideoFrontEnd     image, flow_x, flow_y -> video (L, T, 3, s, s), flow (L, T, 2, s, s), box: what `AudioInpainter(..., video=, flow=)` and
                      `AudioModel.set_inputs(video=, flow=)` take

The rule is stated in full in include/viai_hip.h.  Everything is integer arithmetic up to the one fp32 divide `(q - 127) / 128`, so all results
are exact: the same bits from run to run, and `prepare(...)` has the bits of `batch.frames_prep(resize_u8(...), ...)`.  The box never leaves the
device: the output size is fixed, so nothing on the host needs it.  The resize is OpenCV's 8-bit INTER_LINEAR restated as integer arithmetic;
OpenCV is not a dependency, so parity with it is restated, not pinned.  The reference's JPEG round trip between crop and resize is left out.

A clip whose motion box is smaller than `min_extent` on either axis has `box[4] == 0` (the reference deletes such a clip); the resampling
passes then take the whole frame, which is a choice made here for inference.
"""
from __future__ import annotations

import torch

from . import _lib

BOX_FIELDS = ("w_min", "w_max", "h_min", "h_max", "ok")


def _need_cuda(t, what):
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s: a torch tensor expected, got %s" % (what, type(t).__name__))
    if not t.is_cuda:
        raise _lib.ViaiLibraryError("%s runs on the GPU only (got a %s tensor); no CPU fallback" % (what, t.device))
    if t.dtype != torch.uint8:
        raise TypeError("%s: uint8 expected, got %s" % (what, t.dtype))
    return t


def _frames_view(t, inner):
    """(tensor, frame stride in bytes) of a stack whose frames are contiguous; the first dimension may be any view with a stride of at least one
    frame, everything else is copied"""
    if not (t[0].is_contiguous() and (t.size(0) == 1 or t.stride(0) >= inner)):
        t = t.contiguous()
    return t, (t.stride(0) if t.size(0) > 1 else inner)


def _flows(flow_x, flow_y, what):
    flow_x, flow_y = _need_cuda(flow_x, what), _need_cuda(flow_y, what)
    if flow_x.dim() != 3 or flow_x.shape != flow_y.shape or flow_x.numel() == 0:
        raise ValueError("%s: flow_x and flow_y are (N, H, W), the same shape" % what)
    N, H, W = flow_x.shape
    if H >= 1 << 15 or W >= 1 << 15:
        raise ValueError("%s: H and W below 2^15" % what)
    flow_x, sx = _frames_view(flow_x, H * W)
    flow_y, sy = _frames_view(flow_y, H * W)
    if sx != sy:
        flow_x, flow_y, sx = flow_x.contiguous(), flow_y.contiguous(), H * W
    return flow_x, flow_y, sx, N, H, W


def motion_box(flow_x, flow_y, min_extent=50):
    """flow_x, flow_y (N, H, W) uint8 on the GPU -> int32 (5,) `(w_min, w_max, h_min, h_max, ok)` on the device.  Two launches, no
    synchronisation, no copy to the host.  The stacks may be views along the first dimension (every other frame, a range); frames themselves
    are contiguous or get copied."""
    if int(min_extent) != min_extent or min_extent < 0:
        raise ValueError("motion_box: min_extent is an integer >= 0")
    flow_x, flow_y, stride, N, H, W = _flows(flow_x, flow_y, "motion_box")
    lib = _lib.load()
    from .ops import _stream
    ws = torch.empty(int(lib.viai_motion_box_ws_bytes(H, W)), dtype=torch.uint8, device=flow_x.device)
    box = torch.empty(5, dtype=torch.int32, device=flow_x.device)
    _lib.check(lib.viai_motion_box(flow_x.data_ptr(), flow_y.data_ptr(), stride, N, H, W, int(min_extent), box.data_ptr(), ws.data_ptr(),
                                   _stream()), "viai_motion_box")
    return box


def motion_box_host(flow_x, flow_y, min_extent=50):
    """`motion_box` on the host: (N, H, W) uint8 numpy arrays, the rule pixel by pixel and `find_cluster` as the reference walks it, in plain
    C++.  Returns an int32 numpy array (5,).  Needs the built library, not a GPU."""
    import ctypes as C

    import numpy as np
    if int(min_extent) != min_extent or min_extent < 0:
        raise ValueError("motion_box_host: min_extent is an integer >= 0")
    fx, fy = np.ascontiguousarray(flow_x, dtype=np.uint8), np.ascontiguousarray(flow_y, dtype=np.uint8)
    if fx.ndim != 3 or fx.shape != fy.shape or fx.size == 0:
        raise ValueError("motion_box_host: flow_x and flow_y are (N, H, W), the same shape")
    N, H, W = fx.shape
    box = np.empty(5, dtype=np.int32)
    _lib.check(_lib.load().viai_motion_box_host(fx.ctypes.data_as(C.c_void_p), fy.ctypes.data_as(C.c_void_p), H * W, N, H, W, int(min_extent),
                                                box.ctypes.data_as(C.c_void_p)), "viai_motion_box_host")
    return box


def _host_box(box, H, W, what):
    """four host ints (w_min, w_max, h_min, h_max), validated -> the five ints with ok = 1"""
    b = [int(v) for v in box]
    if len(b) != 4 or any(int(v) != v for v in box):
        raise ValueError("%s: a host box is four ints (w_min, w_max, h_min, h_max)" % what)
    if not (0 <= b[0] < b[1] <= W and 0 <= b[2] < b[3] <= H):
        raise ValueError("%s: box %s is not a non-empty crop inside a %d x %d frame" % (what, b, H, W))
    return b + [1]


def _sources(frames, what):
    """frames: (N, H, W, C) uint8, or a pair (flow_x, flow_y) of (N, H, W) planes -> (src0, src1 or None, frame stride, N, H, W, C)"""
    if isinstance(frames, (tuple, list)):
        if len(frames) != 2:
            raise ValueError("%s: a pair of planes is (flow_x, flow_y)" % what)
        a, b, stride, N, H, W = _flows(frames[0], frames[1], what)
        return a, b, stride, N, H, W, 2
    f = _need_cuda(frames, what)
    if f.dim() != 4 or f.numel() == 0 or not 1 <= f.size(3) <= 4:
        raise ValueError("%s: frames are (N, H, W, C) with C in 1..4, or a pair of (N, H, W) planes" % what)
    N, H, W, C = f.shape
    if H >= 1 << 15 or W >= 1 << 15:
        raise ValueError("%s: H and W below 2^15" % what)
    f, stride = _frames_view(f, H * W * C)
    return f, None, stride, N, H, W, C


def _index(frames_index, N, dev, what):
    if frames_index is None:
        return None, N
    idx = [int(i) for i in frames_index]
    if len(idx) < 1 or any(int(i) != i for i in frames_index) or min(idx) < 0 or max(idx) >= N:
        raise ValueError("%s: frames_index holds at least one int, each in [0, %d)" % (what, N))
    return torch.tensor(idx, dtype=torch.int32, device=dev), len(idx)


def _box_on(box, H, W, dev, what):
    if isinstance(box, torch.Tensor):
        if box.numel() != 5 or box.dtype != torch.int32:
            raise ValueError("%s: a device box is the int32 (5,) tensor of motion_box" % what)
        if not box.is_cuda:
            raise _lib.ViaiLibraryError("%s: the box tensor lives on the GPU (or pass four host ints)" % what)
        return box.contiguous()
    return torch.tensor(_host_box(box, H, W, what), dtype=torch.int32, device=dev)


def _ws(lib, R, dev):
    nbytes = int(lib.viai_video_prep_ws_bytes(int(R)))
    if nbytes < 1:
        raise ValueError("resize to R = %r: 1 <= R <= 8192" % (R,))
    return torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)


def resize_u8(frames, box, R, bgr=False, frames_index=None):
    """Crop `frames` to `box`, pad to a square with grey 127 and resize to R x R: uint8 (n, R, R, C) on the device.  frames: (N, H, W, C) uint8
    on the GPU, or the pair (flow_x, flow_y) of (N, H, W) planes (C = 2).  box: the device tensor of `motion_box`, or four host ints
    (w_min, w_max, h_min, h_max), validated here.  frames_index: host ints, validated here; None: every frame."""
    src0, src1, stride, N, H, W, C = _sources(frames, "resize_u8")
    lib = _lib.load()
    from .ops import _stream
    dev = src0.device
    idx, n = _index(frames_index, N, dev, "resize_u8")
    ws = _ws(lib, R, dev)
    box = _box_on(box, H, W, dev, "resize_u8")
    out = torch.empty((n, int(R), int(R), C), dtype=torch.uint8, device=dev)
    _lib.check(lib.viai_video_resize_u8(src0.data_ptr(), 0 if src1 is None else src1.data_ptr(), stride, N, H, W, C, int(bool(bgr)),
                                        box.data_ptr(), 0 if idx is None else idx.data_ptr(), n, int(R), out.data_ptr(), ws.data_ptr(),
                                        _stream()), "viai_video_resize_u8")
    return out


def resize_u8_host(frames, box, R, bgr=False, frames_index=None):
    """`resize_u8` on the host: frames a (N, H, W, C) uint8 numpy array or a pair of (N, H, W) planes, box five ints (the last is `ok`) or four.
    Returns a uint8 numpy array (n, R, R, C).  Needs the built library, not a GPU."""
    import ctypes as C_

    import numpy as np
    if isinstance(frames, (tuple, list)):
        a, b = (np.ascontiguousarray(p, dtype=np.uint8) for p in frames)
        if a.ndim != 3 or a.shape != b.shape:
            raise ValueError("resize_u8_host: a pair of planes is (flow_x, flow_y), each (N, H, W)")
        (N, H, W), C, pb = a.shape, 2, b.ctypes.data_as(C_.c_void_p)
    else:
        a = np.ascontiguousarray(frames, dtype=np.uint8)
        if a.ndim != 4:
            raise ValueError("resize_u8_host: frames are (N, H, W, C)")
        (N, H, W, C), pb = a.shape, None
    box = [int(v) for v in box]
    box = np.array(box if len(box) == 5 else _host_box(box, H, W, "resize_u8_host"), dtype=np.int32)
    idx, n, pi = None, N, None
    if frames_index is not None:
        idx = np.array([int(i) for i in frames_index], dtype=np.int32)
        if idx.size < 1 or idx.min() < 0 or idx.max() >= N:
            raise ValueError("resize_u8_host: frames_index holds ints in [0, %d)" % N)
        n, pi = idx.size, idx.ctypes.data_as(C_.c_void_p)
    out = np.empty((n, int(R), int(R), C), dtype=np.uint8)
    _lib.check(_lib.load().viai_video_resize_u8_host(a.ctypes.data_as(C_.c_void_p), pb, H * W * (1 if pb is not None else C), N, H, W, C,
                                                     int(bool(bgr)), box.ctypes.data_as(C_.c_void_p), pi, n, int(R),
                                                     out.ctypes.data_as(C_.c_void_p)), "viai_video_resize_u8_host")
    return out


def prepare(frames, box, R, size, crop_x=0, crop_y=0, flip=False, bgr=False, frames_index=None, nchw=False):
    """Crop to the box, pad, resize to R x R, flip left to right, crop rows [crop_x, +size) and columns [crop_y, +size), `(q - 127) / 128`: fp32
    (n, size, size, 4) NHWC4 with channels >= C zero (what ResNet conv1 consumes), or with nchw=True the reference's (n, C, size, size).  Only
    the size x size window is computed.  Bit for bit `batch.frames_prep(resize_u8(frames, box, R, ...), size, crop_x, crop_y, flip, nchw)`."""
    src0, src1, stride, N, H, W, C = _sources(frames, "prepare")
    R, size, crop_x, crop_y = int(R), int(size), int(crop_x), int(crop_y)
    if not (1 <= size <= R and 0 <= crop_x <= R - size and 0 <= crop_y <= R - size):
        raise ValueError("prepare: the %d x %d window at (%d, %d) does not lie inside %d x %d" % (size, size, crop_x, crop_y, R, R))
    lib = _lib.load()
    from .ops import _stream
    dev = src0.device
    idx, n = _index(frames_index, N, dev, "prepare")
    ws = _ws(lib, R, dev)
    box = _box_on(box, H, W, dev, "prepare")
    out = torch.empty((n, C, size, size) if nchw else (n, size, size, 4), dtype=torch.float32, device=dev)
    _lib.check(lib.viai_video_prepare(src0.data_ptr(), 0 if src1 is None else src1.data_ptr(), stride, N, H, W, C, int(bool(bgr)),
                                      box.data_ptr(), 0 if idx is None else idx.data_ptr(), n, R, size, crop_x, crop_y, int(bool(flip)),
                                      int(bool(nchw)), out.data_ptr(), ws.data_ptr(), _stream()), "viai_video_prepare")
    return out


class VideoFrontEnd:
    """image (N, H, W, 3), flow_x and flow_y (N, H, W), uint8 on the GPU -> (video (L, T, 3, s, s), flow (L, T, 2, s, s), box), fp32 and int32
    on the device, s = image_size.

    train=False   resize straight to image_size, no crop, no flip (`sample_data_new`'s eval branch; crop_x, crop_y and flip must be unset).
    train=True    resize to rescale_size, then the caller's crop_x, crop_y, flip (the reference draws them once per item; nothing is drawn here).
    starts, use_image_num   clip l takes frames [starts[l], starts[l] + use_image_num), as `sample_data_new` does; host ints, validated.
                  None: all frames, L = 1.
    bgr           reverse the image's channel axis (the reference's cvtColor of a decoded BGR frame).
    flow_x, flow_y   both None: computed from the image by `optical_flow.flow_u8(image, bgr=bgr, **flow_params)` (TV-L1);
                  exactly one of them is a ValueError.

    Four launches for the box and the tables, two resampling launches; no synchronisation, and the box is never read on the host."""

    def __init__(self, image_size=224, rescale_size=256, min_extent=50):
        if not 1 <= int(image_size) <= int(rescale_size):
            raise ValueError("VideoFrontEnd: 1 <= image_size <= rescale_size")
        self.image_size, self.rescale_size, self.min_extent = int(image_size), int(rescale_size), int(min_extent)

    def __call__(self, image, flow_x=None, flow_y=None, train=False, crop_x=0, crop_y=0, flip=False, starts=None, use_image_num=None, bgr=False,
                 flow_params=None):
        _need_cuda(image, "VideoFrontEnd")
        if (flow_x is None) != (flow_y is None):
            raise ValueError("VideoFrontEnd: flow_x and flow_y come together, or neither (the flow is then computed from the image)")
        if flow_x is None:
            if image.dim() != 4 or image.size(3) != 3 or image.size(0) < 2:
                raise ValueError("VideoFrontEnd: image is (N, H, W, 3) with N >= 2 when the flow is computed from it")
            from .optical_flow import flow_u8
            flow_x, flow_y = flow_u8(image, bgr=bgr, **(flow_params or {}))
        elif flow_params is not None:
            raise ValueError("VideoFrontEnd: flow_params belong to a call without flow_x and flow_y")
        if image.dim() != 4 or image.size(3) != 3 or flow_x.dim() != 3 or tuple(image.shape[:3]) != tuple(flow_x.shape):
            raise ValueError("VideoFrontEnd: image is (N, H, W, 3), flow_x and flow_y are (N, H, W)")
        N, s = image.size(0), self.image_size
        if not train and (crop_x or crop_y or flip):
            raise ValueError("VideoFrontEnd: crop and flip belong to train=True")
        if (starts is None) != (use_image_num is None):
            raise ValueError("VideoFrontEnd: starts and use_image_num come together")
        if starts is None:
            L, T, index = 1, N, None
        else:
            T, st = int(use_image_num), [int(v) for v in starts]
            if T < 1 or len(st) < 1 or min(st) < 0 or max(st) + T > N:
                raise ValueError("VideoFrontEnd: clips [start, start + %d) must lie inside the %d frames" % (T, N))
            L, index = len(st), [v + t for v in st for t in range(T)]
        R = self.rescale_size if train else s
        box = motion_box(flow_x, flow_y, self.min_extent)
        kw = dict(crop_x=crop_x, crop_y=crop_y, flip=flip, frames_index=index, nchw=True)
        video = prepare(image, box, R, s, bgr=bgr, **kw)
        flow = prepare((flow_x, flow_y), box, R, s, **kw)
        return video.view(L, T, 3, s, s), flow.view(L, T, 2, s, s), box
