"""The video front end's rule (include/viai_hip.h) stated in numpy, and the cases the CPU test, the GPU test and
tools/make_video_prep_golden.py share.  Frames come from closed formulas (`oracle.viai_oracle.cf_uniform` plus painted blocks), so the fixture
stores parameters and results only.

    box_rule       S, the mask, the occupied indices, `find_cluster` walked as the reference walks it -> (w_min, w_max, h_min, h_max, ok)
    cluster_closed the closed form the kernel evaluates (first v with v + 5 occupied, ...)
    geo            the crop a box means inside an H x W frame (clamp, whole frame for ok == 0) and its pad offsets
    crop_pad       the crop padded to a square with grey 127
    coef_table     the R-entry table of side -> R
    resize         side x side -> R x R by the integer rule
    resize_rule    frames (+ box, bgr, frames_index) -> uint8 (n, R, R, C): crop_pad + resize per frame
"""
import hashlib

import numpy as np

from oracle import viai_oracle as O

MIN_EXTENT = 50


# ----------------------------------------------------------------------------- the motion box
def occupied(flow_x, flow_y):
    """(occupied columns, occupied rows), ascending int arrays"""
    N = flow_x.shape[0]
    S = np.abs(flow_x.astype(np.int32) - 127).sum(0) + np.abs(flow_y.astype(np.int32) - 127).sum(0)
    mask = S > 2 * N
    return np.flatnonzero(mask.any(0)), np.flatnonzero(mask.any(1))


def cluster_walk(o):
    """`find_cluster` on the ascending list o, as the reference walks it"""
    o = [int(v) for v in o]
    if not o:
        return 0, 0
    has = set(o)
    lo, hi = 0, len(o) - 1
    for _ in range(len(o) - 1):
        if o[lo] + 5 not in has:
            lo += 1
    for _ in range(len(o) - 1):
        if o[hi] - 5 not in has:
            hi -= 1
    mn, mx = o[lo], o[hi]
    return mn, max(mx, mn)


def cluster_closed(o):
    """the same without the walk"""
    o = [int(v) for v in o]
    if not o:
        return 0, 0
    has = set(o)
    mn = next((v for v in o if v + 5 in has), o[-1])
    mx = next((v for v in reversed(o) if v - 5 in has), o[0])
    return mn, max(mx, mn)


def box_rule(flow_x, flow_y, min_extent=MIN_EXTENT, cluster=cluster_walk):
    ow, oh = occupied(flow_x, flow_y)
    w0, w1 = cluster(ow)
    h0, h1 = cluster(oh)
    return np.array([w0, w1, h0, h1, int(w1 - w0 >= min_extent and h1 - h0 >= min_extent)], dtype=np.int32)


# ----------------------------------------------------------------------------- crop and pad
def geo(box, H, W):
    """(x0, y0, cw, ch, side, padx, pady) of a five-int box inside an H x W frame"""
    clamp = lambda v, lo, hi: min(max(int(v), lo), hi)
    w0 = clamp(box[0], 0, W)
    w1 = clamp(box[1], w0, W)
    h0 = clamp(box[2], 0, H)
    h1 = clamp(box[3], h0, H)
    if int(box[4]) == 0 or w1 - w0 < 1 or h1 - h0 < 1:
        w0, w1, h0, h1 = 0, W, 0, H
    cw, ch = w1 - w0, h1 - h0
    side = max(cw, ch)
    return w0, h0, cw, ch, side, (side - cw) // 2, (side - ch) // 2


def crop_pad(img, box):
    """img (H, W) or (H, W, C) -> the crop of `box` padded to (side, side[, C]) with 127: d // 2 in front, d - d // 2 behind"""
    H, W = img.shape[:2]
    x0, y0, cw, ch, side, padx, pady = geo(box, H, W)
    out = np.full((side, side) + img.shape[2:], 127, dtype=np.uint8)
    out[pady:pady + ch, padx:padx + cw] = img[y0:y0 + ch, x0:x0 + cw]
    return out


# ----------------------------------------------------------------------------- resize
def coef_table(side, R):
    """(s, c0, c1): int arrays of R entries"""
    d = np.arange(R, dtype=np.float64)
    f = ((d + 0.5) * (float(side) / float(R)) - 0.5).astype(np.float32)
    fl = np.floor(f)
    s = fl.astype(np.int64)
    a = (f - fl).astype(np.float32)
    lo, hi = s < 0, s >= side - 1
    s = np.where(lo, 0, np.where(hi, side - 1, s))
    a = np.where(lo | hi, np.float32(0), a).astype(np.float32)
    c0 = np.rint((np.float32(1) - a) * np.float32(2048)).astype(np.int64)
    c1 = np.rint(a * np.float32(2048)).astype(np.int64)
    return s, c0, c1


def resize(sq, R):
    """sq (side, side, C) uint8 -> (R, R, C) uint8"""
    side = sq.shape[0]
    assert sq.shape[1] == side and sq.ndim == 3
    s, c0, c1 = coef_table(side, R)
    s1 = np.minimum(s + 1, side - 1)
    p = sq.astype(np.int64)
    h = p[:, s, :] * c0[None, :, None] + p[:, s1, :] * c1[None, :, None]                    # (side, R, C)
    q = (((c0[:, None, None] * (h[s] >> 4)) >> 16) + ((c1[:, None, None] * (h[s1] >> 4)) >> 16) + 2) >> 2
    return np.minimum(q, 255).astype(np.uint8)


def resize_rule(frames, box, R, bgr=False, frames_index=None):
    """frames (N, H, W, C) uint8, or a pair of (N, H, W) planes; box five ints -> uint8 (n, R, R, C)"""
    if isinstance(frames, (tuple, list)):
        frames = np.stack(frames, axis=-1)
    if bgr:
        frames = frames[..., ::-1]
    idx = range(frames.shape[0]) if frames_index is None else frames_index
    return np.stack([resize(crop_pad(frames[i], box), R) for i in idx])


def bilinear_f64(sq, R):
    """float bilinear with half-pixel centres (align_corners=False), fp64: what the integer rule approximates"""
    import torch
    t = torch.from_numpy(sq.astype(np.float64)).permute(2, 0, 1)[None]
    return torch.nn.functional.interpolate(t, size=(R, R), mode="bilinear", align_corners=False)[0].permute(1, 2, 0).numpy()


# ----------------------------------------------------------------------------- frames from closed formulas
def u8(tag, shape):
    """uniform bytes 0 .. 255"""
    return np.floor(O.cf_uniform(tag, shape).numpy().astype(np.float64) * 256.0).astype(np.uint8)


def quiet_flow(tag, shape):
    """bytes in {126, 127, 128}: |v - 127| <= 1, so S <= 2 N everywhere and nothing is in the mask"""
    return (126 + np.floor(O.cf_uniform(tag, shape).numpy().astype(np.float64) * 3.0)).astype(np.uint8)


# name, N, H, W, blocks: (y0, y1, x0, x1) painted with fx = 147 on every frame (S >= 20 N there), quiet elsewhere
CASES = [
    dict(name="one blob", N=3, H=96, W=120, blocks=[(10, 71, 20, 91)]),
    dict(name="blob and an isolated index", N=3, H=96, W=120, blocks=[(5, 86, 20, 81), (93, 94, 110, 111)]),
    dict(name="blob from edge to edge", N=2, H=80, W=100, blocks=[(0, 80, 0, 100)]),
    dict(name="empty mask", N=3, H=64, W=80, blocks=[]),
    dict(name="blob 49 wide", N=3, H=96, W=120, blocks=[(20, 70, 20, 70)]),
    dict(name="one occupied index", N=2, H=64, W=80, blocks=[(31, 32, 47, 48)]),
    dict(name="occupied 3 and 40", N=2, H=64, W=80, blocks=[(3, 4, 3, 4), (40, 41, 40, 41)]),
    dict(name="threshold 2N and 2N+1", N=4, H=64, W=80, blocks=[], exact=True),
]


def case_names():
    return [c["name"] for c in CASES]


def case_by_name(name):
    return next(c for c in CASES if c["name"] == name)


def case_frames(c):
    """(image (N, H, W, 3), flow_x, flow_y (N, H, W)) of a case"""
    N, H, W = c["N"], c["H"], c["W"]
    tag = "video_prep." + c["name"]
    image = u8(tag + ".image", (N, H, W, 3))
    if c.get("exact"):
        fx = np.full((N, H, W), 127, dtype=np.uint8)
        fy = np.full((N, H, W), 127, dtype=np.uint8)
        fx[:, 20, 30] = 129                              # S == 2 N: out
        fx[:, 20, 31] = 129                              # ... and one more on one frame: S == 2 N + 1, in
        fy[0, 20, 31] = 128
        return image, fx, fy
    fx, fy = quiet_flow(tag + ".fx", (N, H, W)), quiet_flow(tag + ".fy", (N, H, W))
    for y0, y1, x0, x1 in c["blocks"]:
        fx[:, y0:y1, x0:x1] = 147
    return image, fx, fy


def digest(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(repr(a.shape).encode() + a.tobytes()).hexdigest()


def random_flows(N, H, W, seed, p=0.004):
    """quiet flows with a few loud pixels: sparse occupied rows and columns, clusters and loners"""
    r = np.random.RandomState(seed)
    fx = r.randint(126, 129, size=(N, H, W)).astype(np.uint8)
    fy = r.randint(126, 129, size=(N, H, W)).astype(np.uint8)
    loud = r.rand(H, W) < p
    fx[:, loud] = 200
    return fx, fy
