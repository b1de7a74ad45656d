"""GPU: the video front end (csrc/video_prep.hip) on the device.  `motion_box` equals the host rule bit for bit; `resize_u8`
equals the numpy resize exactly; `prepare` has the bits of `batch.frames_prep(resize_u8(...))`; `VideoFrontEnd` slices clips as the all-frames
result sliced by hand.  Everything is integer arithmetic or a select followed by the one fp32 divide `frames_prep` already performs, so every
comparison is exact.

Sizes: frames of at most 120 x 130, R at most 256; W = 101 and 90 are odd (rows not 16-byte aligned: the motion pass's byte loads), W = 80 and 96
take its 16-byte loads, W = 300 needs more than one 256-pixel tile along a row."""
import numpy as np
import pytest
import torch

import video_prep_common as V

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.fixture(scope="module")
def clip():
    """one clip for the resampling tests: image (6, 120, 130, 3), flow_x, flow_y (6, 120, 130), numpy and device; made once, never written"""
    image = V.u8("video_prep.gpu.image", (6, 120, 130, 3))
    fx, fy = V.u8("video_prep.gpu.fx", (6, 120, 130)), V.u8("video_prep.gpu.fy", (6, 120, 130))
    return dict(image=image, fx=fx, fy=fy, d_image=dev(image), d_fx=dev(fx), d_fy=dev(fy))


# ----------------------------------------------------------------------------- 1. the motion box
def check_box(fx, fy, min_extent=50, d_fx=None, d_fy=None):
    from viai_amd.video import motion_box, motion_box_host
    got = motion_box(dev(fx) if d_fx is None else d_fx, dev(fy) if d_fy is None else d_fy, min_extent)
    assert got.dtype == torch.int32 and got.is_cuda and tuple(got.shape) == (5,)
    want = motion_box_host(fx, fy, min_extent)
    assert np.array_equal(got.cpu().numpy(), want), (got.cpu().numpy(), want)
    assert np.array_equal(want, V.box_rule(fx, fy, min_extent))
    return want


@pytest.mark.parametrize("name", V.case_names())
def test_motion_box_equals_the_host_rule_on_the_fixture_cases(name, golden_dir):
    import os
    i = V.case_names().index(name)
    _, fx, fy = V.case_frames(V.CASES[i])
    want = check_box(fx, fy)
    assert np.array_equal(want, np.load(os.path.join(golden_dir, "video_prep.npz"))["box%d" % i])


@pytest.mark.parametrize("N,H,W", [(5, 67, 101), (1, 67, 101), (1, 72, 90), (5, 64, 96), (3, 9, 300), (2, 1, 1), (2, 5, 17)])
def test_motion_box_equals_the_host_rule_on_random_flows(N, H, W):
    for seed in range(3):
        fx, fy = V.random_flows(N, H, W, 1000 * N + W + seed, p=0.004 if H * W > 2000 else 0.1)
        for min_extent in (50, 0):
            check_box(fx, fy, min_extent)


def test_motion_box_of_a_view_along_the_first_dimension():
    """every other frame of a stack, and a stack that does not start on a 16-byte boundary: read in place"""
    from viai_amd.video import motion_box
    fx, fy = V.random_flows(10, 64, 96, 77)
    d_fx, d_fy = dev(fx), dev(fy)
    check_box(fx[::2], fy[::2], d_fx=d_fx[::2], d_fy=d_fy[::2])
    check_box(fx[3:7], fy[3:7], d_fx=d_fx[3:7], d_fy=d_fy[3:7])
    flat = torch.zeros(10 * 64 * 96 + 16, dtype=torch.uint8, device="cuda")
    flat[5:5 + 10 * 64 * 96] = d_fx.reshape(-1)                            # 5 bytes off: no 16-byte load is legal, the byte loads take it
    off = flat[5:5 + 10 * 64 * 96].view(10, 64, 96)
    check_box(fx, fy, d_fx=off, d_fy=d_fy)
    want = motion_box(d_fx.permute(0, 2, 1), d_fy.permute(0, 2, 1))        # frames that are not contiguous are copied
    assert np.array_equal(want.cpu().numpy(), V.box_rule(fx.transpose(0, 2, 1), fy.transpose(0, 2, 1)))


# ----------------------------------------------------------------------------- 2. the resize
BOXES = [("odd x0, tall", (31, 80, 3, 110)), ("wide", (4, 126, 40, 91)), ("up-scaling 60", (10, 70, 20, 80)), ("one pixel", (7, 8, 9, 10))]


@pytest.mark.parametrize("what,box", BOXES, ids=[b[0] for b in BOXES])
def test_resize_u8_equals_the_numpy_resize(what, box, clip):
    from viai_amd.video import resize_u8
    box5 = list(box) + [1]
    for R in (224, 256):
        got = resize_u8(clip["d_image"], box, R, frames_index=[0, 5])
        assert got.dtype == torch.uint8 and tuple(got.shape) == (2, R, R, 3)
        assert np.array_equal(got.cpu().numpy(), V.resize_rule(clip["image"], box5, R, frames_index=[0, 5])), (what, R)
    got = resize_u8((clip["d_fx"], clip["d_fy"]), box, 256, frames_index=[2])
    assert np.array_equal(got.cpu().numpy(), V.resize_rule((clip["fx"], clip["fy"]), box5, 256, frames_index=[2])), what
    got = resize_u8(clip["d_image"], box, 224, bgr=True, frames_index=[1])
    assert np.array_equal(got.cpu().numpy(), V.resize_rule(clip["image"], box5, 224, bgr=True, frames_index=[1])), what
    two = clip["d_image"][..., :2].contiguous()
    got = resize_u8(two, box, 224, frames_index=[4])
    assert np.array_equal(got.cpu().numpy(), V.resize_rule(clip["image"][..., :2], box5, 224, frames_index=[4])), what


def test_resize_u8_identity_and_down_scaling():
    from viai_amd.video import resize_u8
    for side, R in ((224, 224), (256, 256), (300, 224), (300, 256)):
        sq = V.u8("video_prep.gpu.square.%d" % side, (1, side, side, 3))
        got = resize_u8(dev(sq), (0, side, 0, side), R).cpu().numpy()
        assert np.array_equal(got[0], V.resize(sq[0], R)), (side, R)
        if side == R:
            assert np.array_equal(got, sq)


def test_resize_u8_takes_the_box_from_the_device(clip):
    from viai_amd.video import resize_u8
    box = torch.tensor([31, 80, 3, 110, 1], dtype=torch.int32, device="cuda")
    assert torch.equal(resize_u8(clip["d_image"], box, 64), resize_u8(clip["d_image"], (31, 80, 3, 110), 64))
    wild = torch.tensor([-50, 1 << 20, 100, 1 << 30, 1], dtype=torch.int32, device="cuda")              # clamped before any address is formed
    assert np.array_equal(resize_u8(clip["d_image"], wild, 64).cpu().numpy(), V.resize_rule(clip["image"], [0, 130, 100, 120, 1], 64))
    with pytest.raises(ValueError):
        resize_u8(clip["d_image"], (31, 131, 3, 110), 64)                  # host ints are validated: 131 > W
    with pytest.raises(ValueError):
        resize_u8(clip["d_image"], (31, 80, 3, 110), 64, frames_index=[6])


# ----------------------------------------------------------------------------- 3. prepare is frames_prep of resize_u8
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("nchw", [False, True])
def test_prepare_has_the_bits_of_frames_prep_of_resize_u8(flip, nchw, clip):
    from viai_amd.batch import frames_prep
    from viai_amd.video import prepare, resize_u8
    R, size, box = 256, 224, (31, 80, 3, 110)
    for frames, C in ((clip["d_image"], 3), ((clip["d_fx"], clip["d_fy"]), 2)):
        mid = resize_u8(frames, box, R, frames_index=[1, 4])
        for crop in ((0, 0), (R - size, R - size), (5, 17)):
            got = prepare(frames, box, R, size, crop_x=crop[0], crop_y=crop[1], flip=flip, frames_index=[1, 4], nchw=nchw)
            want = frames_prep(mid, size, crop[0], crop[1], flip, nchw=nchw)
            assert tuple(got.shape) == ((2, C, size, size) if nchw else (2, size, size, 4))
            assert same_bits(got, want), (C, crop, flip, nchw)
            if not nchw:
                assert (got[..., C:].contiguous().view(torch.int32) == 0).all()            # the pad channels are +0.0 exactly
    # straight to the output size (the eval branch): nothing to crop
    got = prepare(clip["d_image"], box, 224, 224, bgr=True, frames_index=[0])
    assert same_bits(got, frames_prep(resize_u8(clip["d_image"], box, 224, bgr=True, frames_index=[0]), 224))
    with pytest.raises(ValueError):
        prepare(clip["d_image"], box, 224, 225)
    with pytest.raises(ValueError):
        prepare(clip["d_image"], box, 256, 224, crop_x=33)


def test_frames_index_repeated_and_reversed_equals_the_per_frame_calls(clip):
    from viai_amd.video import prepare, resize_u8
    box, index = (4, 126, 40, 91), [5, 0, 0, 3, 5, 1]
    got = prepare(clip["d_image"], box, 64, 56, crop_x=3, crop_y=8, flip=True, frames_index=index)
    for k, i in enumerate(index):
        assert same_bits(got[k:k + 1], prepare(clip["d_image"], box, 64, 56, crop_x=3, crop_y=8, flip=True, frames_index=[i])), (k, i)
    assert same_bits(prepare(clip["d_image"], box, 64, 56), prepare(clip["d_image"], box, 64, 56, frames_index=range(6)))
    every_other = clip["d_image"][::2]                                    # a view along the first dimension is read in place
    assert torch.equal(resize_u8(every_other, box, 64), resize_u8(clip["d_image"], box, 64, frames_index=[0, 2, 4]))


def test_a_box_that_is_not_ok_gives_the_whole_frame(clip):
    from viai_amd.video import VideoFrontEnd, motion_box, prepare
    c = V.case_by_name("blob 49 wide")
    image, fx, fy = V.case_frames(c)
    box = motion_box(dev(fx), dev(fy))
    assert box.cpu().tolist() == [20, 69, 20, 69, 0]
    got = prepare(dev(image), box, 64, 64)
    assert same_bits(got, prepare(dev(image), (0, c["W"], 0, c["H"]), 64, 64))
    video, flow, b = VideoFrontEnd(64, 64)(dev(image), dev(fx), dev(fy))
    assert b.cpu().tolist()[4] == 0 and same_bits(video[0], prepare(dev(image), (0, c["W"], 0, c["H"]), 64, 64, nchw=True))


# ----------------------------------------------------------------------------- 4. VideoFrontEnd
def test_video_front_end_clips_are_slices_of_the_all_frames_result():
    from viai_amd.video import VideoFrontEnd, motion_box, prepare
    c = V.case_by_name("blob and an isolated index")
    image, fx, fy = V.case_frames(dict(c, N=7))
    d_image, d_fx, d_fy = dev(image), dev(fx), dev(fy)
    front = VideoFrontEnd(image_size=56, rescale_size=64)
    video, flow, box = front(d_image, d_fx, d_fy)                         # eval: all frames, L = 1
    assert tuple(video.shape) == (1, 7, 3, 56, 56) and tuple(flow.shape) == (1, 7, 2, 56, 56) and video.dtype == torch.float32
    assert box.cpu().tolist() == [20, 80, 5, 85, 1] and torch.equal(box, motion_box(d_fx, d_fy))
    assert same_bits(video[0], prepare(d_image, box, 56, 56, nchw=True)) and same_bits(flow[0], prepare((d_fx, d_fy), box, 56, 56, nchw=True))
    v2, f2, _ = front(d_image, d_fx, d_fy, starts=[4, 0, 2], use_image_num=3)
    assert tuple(v2.shape) == (3, 3, 3, 56, 56) and tuple(f2.shape) == (3, 3, 2, 56, 56)
    for l, s in enumerate([4, 0, 2]):
        assert same_bits(v2[l], video[0, s:s + 3]) and same_bits(f2[l], flow[0, s:s + 3]), (l, s)
    # train: through rescale_size with the caller's crop and flip
    vt, ft, _ = front(d_image, d_fx, d_fy, train=True, crop_x=2, crop_y=7, flip=True, starts=[1], use_image_num=2, bgr=True)
    assert same_bits(vt[0], prepare(d_image, box, 64, 56, crop_x=2, crop_y=7, flip=True, bgr=True, frames_index=[1, 2], nchw=True))
    assert same_bits(ft[0], prepare((d_fx, d_fy), box, 64, 56, crop_x=2, crop_y=7, flip=True, frames_index=[1, 2], nchw=True))
    for bad in (dict(starts=[5], use_image_num=3), dict(starts=[-1], use_image_num=2), dict(starts=[0]), dict(crop_x=1)):
        with pytest.raises(ValueError):
            front(d_image, d_fx, d_fy, **bad)


def test_a_cpu_tensor_raises():
    from viai_amd._lib import ViaiLibraryError
    from viai_amd.video import VideoFrontEnd, motion_box, prepare
    f = torch.zeros(2, 8, 8, dtype=torch.uint8)
    with pytest.raises(ViaiLibraryError):
        motion_box(f, f)
    with pytest.raises(ViaiLibraryError):
        prepare(torch.zeros(2, 8, 8, 3, dtype=torch.uint8), (0, 8, 0, 8), 4, 4)
    with pytest.raises(ViaiLibraryError):
        VideoFrontEnd(4, 4)(torch.zeros(2, 8, 8, 3, dtype=torch.uint8).cuda(), f, f)
