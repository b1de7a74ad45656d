"""GPU: optical flow on the device (csrc/optical_flow.hip).  The kernels and the host mirror call the same per-pixel functions,
so `tvl1` equals `tvl1_host` bit for bit, fp32 flow and uint8 maps alike; the result does not depend on how many iterations a launch runs
(the test of the LDS halo), on the number of pairs in a pass or on the stack's layout; `VideoFrontEnd(image)` is `VideoFrontEnd(image,
*flow_u8(image))`; and refused calls return before any launch.

Sizes: at most 96 x 128, three frames, scales=3, warps=2, iterations=7 unless stated.  17 x 23 is smaller than a tile and has one level;
70 x 131 has three levels with odd sizes on the way; 32 x 32 and 33 x 33 are one tile and one tile + 1 on both axes."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import optical_flow_common as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tile():
    text = open(os.path.join(ROOT, "include", "viai_hip.h")).read()
    return tuple(int(re.search(r"#define\s+VIAI_FLOW_TILE_%s\s+(\d+)" % a, text).group(1)) for a in "HW")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32 if t.dtype == torch.float32 else np.uint8)


def same(a, b):
    a, b = (bits(t) if isinstance(t, torch.Tensor) else (t.view(np.uint32) if t.dtype == np.float32 else t) for t in (a, b))
    return a.shape == b.shape and np.array_equal(a, b)


@pytest.fixture(scope="module")
def clip():
    """three colour frames at 70 x 131 with a moving texture, the host mirror's flow of them at K = 1; made once, never written"""
    from viai_amd.optical_flow import tvl1_host
    frames = F.rgb_of(F.texture(3, 70, 131, (0.8, -0.6), seed=0))
    return dict(frames=frames, d_frames=dev(frames), host=tvl1_host(frames, iters_per_launch=1, **F.QUICK))


TH, TW = tile()


# ----------------------------------------------------------------------------- 1. device == host
@pytest.mark.parametrize("H,W", [(17, 23), (70, 131), (TH, TW), (TH + 1, TW + 1), (TH, TW + 1), (TH + 1, TW)])
def test_device_equals_the_host_mirror_bit_for_bit(H, W, clip):
    from viai_amd.optical_flow import encode_u8, encode_u8_host, flow_u8, tvl1, tvl1_host
    if (H, W) == (70, 131):
        frames, d_frames, want = clip["frames"], clip["d_frames"], clip["host"]
    else:
        frames = F.texture(3, H, W, (0.8, -0.6), seed=H + W)
        d_frames, want = dev(frames), tvl1_host(frames, **F.QUICK)
    got = tvl1(d_frames, **F.QUICK)
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == (2, 2, H, W)
    assert float(np.abs(want).max()) > 0.1
    assert same(got, want), float(np.abs(got.cpu().numpy() - want).max())
    fx, fy = encode_u8(got)
    wx, wy = encode_u8_host(want)
    assert tuple(fx.shape) == (3, H, W) and same(fx, wx) and same(fy, wy)
    gx, gy = flow_u8(d_frames, **F.QUICK)
    assert same(gx, wx) and same(gy, wy)
    nx, _ = encode_u8(got, bound=2.0, pad_last=False)                     # a bound the flow exceeds: both clamps on the device
    assert tuple(nx.shape) == (2, H, W) and same(nx, encode_u8_host(want, bound=2.0, pad_last=False)[0])


def test_bgr_and_grey_inputs_equal_the_host_mirror(clip):
    from viai_amd.optical_flow import tvl1, tvl1_host
    assert same(tvl1(clip["d_frames"], bgr=True, **F.QUICK), tvl1_host(clip["frames"], bgr=True, **F.QUICK))
    grey = np.ascontiguousarray(clip["frames"][..., 1])
    assert same(tvl1(dev(grey), **F.QUICK), tvl1_host(grey, **F.QUICK))


# ----------------------------------------------------------------------------- 2. independence of K
@pytest.mark.parametrize("K", [1, 2, 3, 8])
def test_the_result_does_not_depend_on_iters_per_launch(K, clip):
    """iterations = 7: K = 2 and 3 leave a remainder launch of 1, K = 8 is one launch of 7 whose halo is wider than what is left of the
    coarsest level (18 x 33) beside a tile"""
    from viai_amd.optical_flow import tvl1
    assert same(tvl1(clip["d_frames"], iters_per_launch=K, **F.QUICK), clip["host"])


def test_default_parameters_at_every_k_agree():
    """30 iterations, 5 warps: K = 4 divides into 7 launches of 4 and one of 2, K = 8 into 3 of 8 and one of 6"""
    from viai_amd.optical_flow import tvl1
    d = dev(F.texture(2, 40, 72, (1.5, -0.75), seed=4))
    one = tvl1(d, iters_per_launch=1, scales=2)
    for K in (4, 8):
        assert same(tvl1(d, iters_per_launch=K, scales=2), one), K
    assert F.epe_interior(one[0].cpu().numpy().astype(np.float64), (1.5, -0.75)) < 0.1


# ----------------------------------------------------------------------------- 3. independence of the stack
def test_a_pair_is_the_same_alone_in_a_stack_and_in_passes_of_one(clip):
    from viai_amd.optical_flow import tvl1
    d = clip["d_frames"]
    whole = tvl1(d, **F.QUICK)
    assert same(whole, clip["host"])
    assert same(tvl1(d[1:3], **F.QUICK)[0], clip["host"][1])
    assert same(tvl1(d[0:2], **F.QUICK)[0], clip["host"][0])
    assert same(tvl1(d, pairs_per_pass=1, **F.QUICK), clip["host"])


def test_a_strided_view_equals_its_contiguous_copy():
    from viai_amd.optical_flow import tvl1, tvl1_host
    frames = F.texture(5, 35, 51, (0.4, 0.3), seed=6)
    d = dev(frames)
    view = d[::2]
    assert not view.is_contiguous()
    got = tvl1(view, **F.QUICK)
    assert same(got, tvl1(view.contiguous(), **F.QUICK))
    assert same(got, tvl1_host(frames[::2], **F.QUICK))
    assert same(tvl1(d[1:4], pairs_per_pass=1, **F.QUICK), tvl1_host(frames[1:4], **F.QUICK))


# ----------------------------------------------------------------------------- 4. the video front end without flow maps
def test_video_front_end_computes_the_flow_it_is_not_given():
    from viai_amd.optical_flow import flow_u8
    from viai_amd.video import VideoFrontEnd
    image = dev(F.rgb_of(F.texture(4, 96, 128, (1.5, -0.75), seed=8)))
    fe = VideoFrontEnd(image_size=32, rescale_size=40, min_extent=10)
    fx, fy = flow_u8(image, **F.QUICK)
    assert tuple(fx.shape) == (4, 96, 128)
    a = fe(image, flow_params=F.QUICK)
    b = fe(image, fx, fy)
    for x, y in zip(a, b):
        assert same(x, y) if x.dtype == torch.float32 else torch.equal(x, y)
    video, flow, box = a
    assert tuple(video.shape) == (1, 4, 3, 32, 32) and tuple(flow.shape) == (1, 4, 2, 32, 32) and tuple(box.shape) == (5,)
    assert box.cpu().tolist()[4] == 1                                     # the whole texture moves
    c = fe(image, train=True, crop_x=3, crop_y=5, flip=True, starts=[0, 1], use_image_num=3, bgr=True, flow_params=F.QUICK)
    gx, gy = flow_u8(image, bgr=True, **F.QUICK)
    d = fe(image, gx, gy, train=True, crop_x=3, crop_y=5, flip=True, starts=[0, 1], use_image_num=3, bgr=True)
    assert tuple(c[0].shape) == (2, 3, 3, 32, 32) and tuple(c[1].shape) == (2, 3, 2, 32, 32)
    assert same(c[0], d[0]) and same(c[1], d[1]) and torch.equal(c[2], d[2])
    assert same(fe(image, flow_x=fx, flow_y=fy)[1], b[1])                 # explicit-flow calls, by keyword or position, are what they were
    with pytest.raises(ValueError):
        fe(image, fx)
    with pytest.raises(ValueError):
        fe(image, flow_y=fy)
    with pytest.raises(ValueError):
        fe(image, fx, fy, flow_params=F.QUICK)


def test_the_blocks_are_what_the_model_takes():
    from viai_amd.video import VideoFrontEnd
    image = dev(F.rgb_of(F.texture(4, 96, 128, (1.5, -0.75), seed=8)))
    video, flow, _ = VideoFrontEnd(image_size=224, rescale_size=256, min_extent=10)(image, flow_params=F.QUICK)
    assert tuple(video.shape) == (1, 4, 3, 224, 224) and tuple(flow.shape) == (1, 4, 2, 224, 224)
    assert video.dtype == flow.dtype == torch.float32 and video.is_contiguous() and flow.is_contiguous()
    assert float(flow.abs().max()) <= 1.0 and float(flow.std()) > 0       # (q - 127) / 128 of maps that are not flat


# ----------------------------------------------------------------------------- 5. refusals on the device
def test_device_entry_points_refuse_before_any_launch():
    from viai_amd import _lib
    lib = _lib.load()
    H, W = 20, 24
    frames = torch.zeros(3, H, W, 3, dtype=torch.uint8, device="cuda")
    flow = torch.full((2, 2, H, W), 7.0, device="cuda")
    ws = torch.zeros(int(lib.viai_optical_flow_ws_bytes(2, H, W, 3)) // 4, dtype=torch.float32, device="cuda")
    fx = torch.full((3, H, W), 9, dtype=torch.uint8, device="cuda")
    fy = fx.clone()
    nan = float("nan")
    torch.cuda.synchronize()

    def call(frames=frames.data_ptr(), stride=H * W * 3, N=3, H=H, W=W, Cn=3, tau=0.25, lam=0.15, theta=0.3, scales=3, warps=1, iterations=2, ipl=4,
             flow=flow.data_ptr(), ws=ws.data_ptr()):
        return lib.viai_optical_flow(frames, stride, N, H, W, Cn, 0, tau, lam, theta, scales, warps, iterations, ipl, flow, ws, None)

    bad = [dict(frames=None), dict(flow=None), dict(ws=None), dict(N=1), dict(H=0), dict(W=0), dict(H=1 << 15), dict(W=1 << 15),
           dict(stride=H * W * 3 - 1), dict(Cn=2), dict(scales=0), dict(warps=0), dict(iterations=0), dict(ipl=0), dict(ipl=9)]
    for name in ("tau", "lam", "theta"):
        bad += [{name: 0.0}, {name: -1.0}, {name: nan}]
    for kw in bad:
        assert call(**kw) == 1, kw

    def enc(flow=flow.data_ptr(), pairs=2, H=H, W=W, bound=20.0, fx=fx.data_ptr(), fy=fy.data_ptr()):
        return lib.viai_flow_encode_u8(flow, pairs, H, W, bound, 1, fx, fy, None)

    for kw in (dict(flow=None), dict(fx=None), dict(fy=None), dict(pairs=0), dict(H=0), dict(W=1 << 15), dict(bound=0.0), dict(bound=nan)):
        assert enc(**kw) == 1, kw
    torch.cuda.synchronize()                                              # no error state is left in HIP, and nothing was written
    assert bool((flow == 7.0).all()) and bool((fx == 9).all()) and bool((ws == 0).all())
    assert call() == 0 and enc() == 0
    torch.cuda.synchronize()
    assert bool((flow == 0.0).all()) and bool((fx == 128).all()) and bool((fy == 128).all())
