"""CPU: the video front end's rule (include/viai_hip.h) without a device.  The numpy statement of the rule equals what the
reference's own `find_cluster` / `crop_image` / `padding_square` gave on the shared cases (tests/golden/video_prep.npz); `motion_box_host` and
`resize_u8_host` (plain C++) equal the numpy rule exactly; the integer resize has the identity and constant properties and stays within one
grey level of fp64 bilinear; and every entry point refuses bad arguments before any launch, so also here."""
import json
import os

import numpy as np
import pytest
import torch

import video_prep_common as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1                                                               # hipErrorInvalidValue


@pytest.fixture(scope="module")
def lib():
    from viai_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "video_prep.npz"))


# ----------------------------------------------------------------------------- 1. the numpy rule is the reference's
def test_the_fixture_was_made_from_these_cases(golden):
    assert json.loads(str(golden["cases"])) == json.loads(json.dumps(V.CASES))


@pytest.mark.parametrize("i", range(len(V.CASES)), ids=V.case_names())
def test_numpy_rule_equals_the_reference_boxes_and_pads(golden, i):
    image, fx, fy = V.case_frames(V.CASES[i])
    want = golden["box%d" % i]
    assert np.array_equal(V.box_rule(fx, fy), want), (V.box_rule(fx, fy), want)
    assert np.array_equal(V.box_rule(fx, fy, cluster=V.cluster_closed), want)                # the closed form the kernel evaluates
    shapes, digests = golden["shapes%d" % i], golden["digests%d" % i]
    w0, w1, h0, h1 = (int(v) for v in want[:4])
    planes = (image[0], fx[0], fy[0], image[-1]) if w1 > w0 and h1 > h0 else ()
    assert len(planes) == len(digests)
    for plane, shape, dig in zip(planes, shapes, digests):
        padded = V.crop_pad(plane, [w0, w1, h0, h1, 1])                   # the reference pads whatever it cropped; ok is tested above
        assert list(padded.shape) == [int(s) for s in shape[:padded.ndim]]
        assert V.digest(padded) == str(dig)


def test_the_cases_say_what_their_names_say(golden):
    box = {c["name"]: golden["box%d" % i].tolist() for i, c in enumerate(V.CASES)}
    assert box["one blob"] == [20, 90, 10, 70, 1]
    assert box["blob and an isolated index"] == [20, 80, 5, 85, 1]        # the loner at column 110 / row 93 is walked away from
    assert box["blob from edge to edge"] == [0, 99, 0, 79, 1]
    assert box["empty mask"] == [0, 0, 0, 0, 0]
    assert box["blob 49 wide"] == [20, 69, 20, 69, 0]
    assert box["one occupied index"] == [47, 47, 31, 31, 0]
    assert box["occupied 3 and 40"] == [40, 40, 40, 40, 0]                # min walks to 40, max walks to 3, then max = min
    assert box["threshold 2N and 2N+1"] == [31, 31, 20, 20, 0]            # column 30 holds S == 2 N and is out


def test_closed_form_of_find_cluster_equals_the_walk():
    r = np.random.RandomState(5)
    for trial in range(400):
        L = int(r.randint(1, 60))
        o = np.flatnonzero(r.rand(L) < r.choice([0.05, 0.2, 0.5, 0.9]))
        assert V.cluster_closed(o) == V.cluster_walk(o), o
    for o in ([], [0], [7], [3, 40], [0, 5], [0, 4], [0, 5, 6], [1, 2, 3, 9, 14, 30], [0, 1, 2, 3, 4], [10, 15, 16, 21, 40]):
        assert V.cluster_closed(o) == V.cluster_walk(o), o


# ----------------------------------------------------------------------------- 2. the host functions are the numpy rule
@pytest.mark.parametrize("name", V.case_names())
def test_motion_box_host_equals_the_numpy_rule_on_the_fixture_cases(name, lib):
    from viai_amd.video import motion_box_host
    _, fx, fy = V.case_frames(V.case_by_name(name))
    got = motion_box_host(fx, fy)
    assert got.dtype == np.int32 and np.array_equal(got, V.box_rule(fx, fy)), (got, V.box_rule(fx, fy))


@pytest.mark.parametrize("N", [1, 5])
def test_motion_box_host_equals_the_numpy_rule_on_random_flows(N, lib):
    from viai_amd.video import motion_box_host
    for seed in range(6):
        fx, fy = V.random_flows(N, 72, 90, 100 * N + seed)
        for min_extent in (50, 10, 0):
            want = V.box_rule(fx, fy, min_extent)
            assert np.array_equal(motion_box_host(fx, fy, min_extent), want), (N, seed, min_extent, want)


SIDES = (1, 3, 50, 67, 101, 224, 256, 300)


@pytest.fixture(scope="module")
def squares():
    """side -> (side, side, 3) uniform bytes, made once"""
    return {s: V.u8("video_prep.square.%d" % s, (s, s, 3)) for s in SIDES}


@pytest.mark.parametrize("R", [224, 256])
@pytest.mark.parametrize("side", SIDES)
def test_resize_u8_host_equals_the_numpy_resize(side, R, squares, lib):
    from viai_amd.video import resize_u8_host
    sq = squares[side]
    for C in (2, 3):
        img = np.ascontiguousarray(sq[None, :, :, :C])
        got = resize_u8_host(img, [0, side, 0, side, 1], R)
        assert got.shape == (1, R, R, C) and got.dtype == np.uint8
        assert np.array_equal(got[0], V.resize(img[0], R)), (side, R, C)
    planes = (np.ascontiguousarray(sq[None, :, :, 0]), np.ascontiguousarray(sq[None, :, :, 1]))
    assert np.array_equal(resize_u8_host(planes, [0, side, 0, side, 1], R), resize_u8_host(np.ascontiguousarray(sq[None, :, :, :2]),
                                                                                           [0, side, 0, side, 1], R))
    bgr = resize_u8_host(np.ascontiguousarray(sq[None]), [0, side, 0, side, 1], R, bgr=True)
    assert np.array_equal(bgr[0], V.resize(sq, R)[..., ::-1])


def test_resize_is_the_identity_when_side_equals_R(squares, lib):
    from viai_amd.video import resize_u8_host
    for side in (224, 256):
        sq = squares[side]
        assert np.array_equal(V.resize(sq, side), sq)
        assert np.array_equal(resize_u8_host(sq[None], [0, side, 0, side, 1], side)[0], sq)


def test_resize_keeps_constant_images_constant(lib):
    from viai_amd.video import resize_u8_host
    for side in (1, 3, 50, 67, 101, 300):
        for value in (0, 1, 127, 254, 255):
            sq = np.full((1, side, side, 2), value, dtype=np.uint8)
            for R in (224, 256):
                assert (V.resize(sq[0], R) == value).all(), (side, value, R)
                assert (resize_u8_host(sq, [0, side, 0, side, 1], R) == value).all(), (side, value, R)


@pytest.mark.parametrize("R", [224, 256])
def test_resize_stays_within_one_grey_level_of_fp64_bilinear(R, squares):
    """The bound is 1.0 grey level: rounding the result to a byte costs up to 0.5, the 11-bit coefficients and the two truncating shifts the
    rest.  On these images the worst difference measured is 0.81.  A failure means the restatement is wrong, not the bound."""
    for side in SIDES:
        d = np.abs(V.resize(squares[side], R).astype(np.float64) - V.bilinear_f64(squares[side], R)).max()
        print("side %3d -> R %d: max |integer - fp64 bilinear| = %.4f" % (side, R, d))
        assert d < 1.0, (side, R, d)


def test_pad_offsets_for_a_tall_and_a_wide_box(lib):
    """written out by hand: a 30 x 17 crop (tall) gets 6 columns of 127 in front and 7 behind; a 12 x 31 crop (wide) gets 9 rows and 10"""
    from viai_amd.video import resize_u8_host
    img = V.u8("video_prep.pad", (1, 40, 50, 3))
    img[img == 127] = 126                                                 # so that 127 marks the pad
    tall = V.crop_pad(img[0], [5, 22, 3, 33, 1])
    assert tall.shape == (30, 30, 3) and (tall[:, :6] == 127).all() and (tall[:, 23:] == 127).all()
    assert np.array_equal(tall[:, 6:23], img[0, 3:33, 5:22])
    wide = V.crop_pad(img[0], [10, 41, 20, 32, 1])
    assert wide.shape == (31, 31, 3) and (wide[:9] == 127).all() and (wide[21:] == 127).all()
    assert np.array_equal(wide[9:21], img[0, 20:32, 10:41])
    # side == R makes the resize the identity, so the host call shows its own pad
    assert np.array_equal(resize_u8_host(img, [5, 22, 3, 33], 30)[0], tall)
    assert np.array_equal(resize_u8_host(img, [10, 41, 20, 32], 31)[0], wide)
    # ok == 0, and a box that is empty after the clamp, mean the whole frame (50 wide, 40 high: 5 rows of pad in front and behind)
    whole = V.crop_pad(img[0], [0, 50, 0, 40, 1])
    assert whole.shape == (50, 50, 3) and (whole[:5] == 127).all() and (whole[45:] == 127).all()
    for box in ([5, 22, 3, 33, 0], [60, 70, 3, 33, 1], [22, 5, 3, 33, 1], [0, 0, 0, 0, 0]):
        assert np.array_equal(V.crop_pad(img[0], box), whole)
        assert np.array_equal(resize_u8_host(img, box, 50)[0], whole), box
    # a box that sticks out of the frame is clamped to it
    assert np.array_equal(resize_u8_host(img, [30, 999, -4, 33, 1], 33)[0], V.crop_pad(img[0], [30, 50, 0, 33, 1]))


def test_frames_index_on_the_host(lib):
    from viai_amd.video import resize_u8_host
    img = V.u8("video_prep.index", (4, 20, 24, 3))
    got = resize_u8_host(img, [2, 20, 1, 19], 16, frames_index=[3, 0, 0, 2])
    assert np.array_equal(got, V.resize_rule(img, [2, 20, 1, 19, 1], 16, frames_index=[3, 0, 0, 2]))
    with pytest.raises(ValueError):
        resize_u8_host(img, [2, 20, 1, 19], 16, frames_index=[4])
    with pytest.raises(ValueError):
        resize_u8_host(img, [2, 20, 1, 41], 16)                           # a host box is validated: 41 > H


# ----------------------------------------------------------------------------- 3. the Python entry points check their arguments
def test_python_entry_points_refuse_cpu_tensors_and_bad_arguments():
    import viai_amd
    from viai_amd import video
    from viai_amd._lib import ViaiLibraryError
    assert viai_amd.VideoFrontEnd is video.VideoFrontEnd
    f = torch.zeros(2, 8, 8, dtype=torch.uint8)
    img = torch.zeros(2, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(ViaiLibraryError):
        video.motion_box(f, f)
    with pytest.raises(ViaiLibraryError):
        video.resize_u8(img, [0, 8, 0, 8], 4)
    with pytest.raises(ViaiLibraryError):
        video.prepare(img, [0, 8, 0, 8], 4, 4)
    with pytest.raises(ViaiLibraryError):
        video.VideoFrontEnd(4, 4)(img, f, f)
    with pytest.raises(ValueError):
        video.VideoFrontEnd(image_size=256, rescale_size=224)
    with pytest.raises(ValueError):
        video.motion_box_host(np.zeros((2, 8, 8), np.uint8), np.zeros((2, 8, 9), np.uint8))
    with pytest.raises(ValueError):
        video.motion_box_host(np.zeros((2, 8, 8), np.uint8), np.zeros((2, 8, 8), np.uint8), min_extent=-1)


# ----------------------------------------------------------------------------- 4. refusals, before any launch
def test_every_refusal_is_invalid_value_without_a_device(lib):
    """the pointers are never dereferenced by a refused call: small fake addresses, aligned as the calls want them"""
    a, b, box, out, ws = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000

    def motion(fx=a, fy=b, stride=48 * 64, N=3, H=48, W=64, min_extent=50, box=box, ws=ws, host=False):
        if host:
            return lib.viai_motion_box_host(fx, fy, stride, N, H, W, min_extent, box)
        return lib.viai_motion_box(fx, fy, stride, N, H, W, min_extent, box, ws, None)

    def resize(src0=a, src1=None, stride=48 * 64 * 3, N=3, H=48, W=64, C=3, bgr=0, box=box, index=None, n=3, R=32, out=out, ws=ws, host=False):
        if host:
            return lib.viai_video_resize_u8_host(src0, src1, stride, N, H, W, C, bgr, box, index, n, R, out)
        return lib.viai_video_resize_u8(src0, src1, stride, N, H, W, C, bgr, box, index, n, R, out, ws, None)

    def prepare(src0=a, src1=None, stride=48 * 64 * 3, N=3, H=48, W=64, C=3, bgr=0, box=box, index=None, n=3, R=32, size=28, crop_x=0, crop_y=0,
                flip=0, nchw=0, out=out, ws=ws):
        return lib.viai_video_prepare(src0, src1, stride, N, H, W, C, bgr, box, index, n, R, size, crop_x, crop_y, flip, nchw, out, ws, None)

    big = 1 << 15
    for kw in (dict(fx=None), dict(fy=None), dict(box=None), dict(N=0), dict(N=-1), dict(N=(1 << 22) + 1), dict(H=0), dict(W=0), dict(H=-3),
               dict(H=big, stride=big * 64), dict(W=big, stride=big * 48), dict(stride=48 * 64 - 1), dict(min_extent=-1)):
        assert motion(**kw) == INVALID, kw
        assert motion(host=True, **kw) == INVALID, kw
    assert motion(ws=None) == INVALID
    shared = (dict(src0=None), dict(box=None), dict(out=None), dict(C=0), dict(C=5, stride=48 * 64 * 5), dict(C=-1), dict(src1=b, C=3),
              dict(N=0), dict(N=-2), dict(n=0), dict(n=4), dict(H=0), dict(W=0), dict(H=big, stride=big * 64 * 3), dict(W=big, stride=big * 48 * 3),
              dict(R=0), dict(R=(1 << 13) + 1), dict(stride=48 * 64 * 3 - 1), dict(src1=b, C=2, stride=48 * 64 - 1))
    for kw in shared:
        assert resize(**kw) == INVALID, kw
        assert resize(host=True, **kw) == INVALID, kw
        assert prepare(**kw) == INVALID, kw
    assert resize(ws=None) == INVALID and prepare(ws=None) == INVALID and resize(ws=ws + 4) == INVALID
    for kw in (dict(size=0), dict(size=33), dict(size=-1), dict(crop_x=-1), dict(crop_y=-1), dict(crop_x=5), dict(crop_y=5),
               dict(size=32, crop_x=1), dict(crop_x=1 << 30), dict(out=out + 4)):
        assert prepare(**kw) == INVALID, kw
    assert lib.viai_motion_box_ws_bytes(0, 64) == 0 and lib.viai_motion_box_ws_bytes(48, big) == 0
    assert lib.viai_motion_box_ws_bytes(48, 64) == 12 * 64 + 1 * 48 and lib.viai_motion_box_ws_bytes(5, 257) == 2 * 257 + 2 * 5
    assert lib.viai_video_prep_ws_bytes(0) == 0 and lib.viai_video_prep_ws_bytes((1 << 13) + 1) == 0
    assert lib.viai_video_prep_ws_bytes(224) == 4 * (8 + 2 * 224)
