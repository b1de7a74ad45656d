"""Every conv launch of the timed step, at its own shape, against fp64.

CENSUS: one `optimize_parameters` step of the benchmark's model (BASELINE.json configs[1]: 16 x 256 x 256, and configs[3]: the
vision-infused step with a 3-scale D, 16 clips of 64 + 64 frames of 224 x 224) runs with every launching entry point of the library that
takes a conv descriptor wrapped (the technique of bench.py KernelTimer / StepFloor, without the timing).  Each call is recorded by value:
entry point, the 17 descriptor fields, the kernel family the library reports (`viai_conv2d_last_kernel`, read on the calling thread right
after the call), act / accumulate / P16 flags and which optional pointers were set.

REPLAY: each distinct launch of the nine pure-conv entry points is called again, same descriptor and flags, on fresh operands (pre-split
ones through the BatchNorm producer with the step's bound rule), and must report the census family -- the replay reached the kernel the
step ran.  Truth is torch in fp64 on the CPU on the DECODED operands (P16 storage error is not the kernel's).  The pre-split inputs are what
select the loader / consumer kernels of csrc/conv_halo_dma.hip; tests/test_fullsize_gpu.py feeds fp32 tensors and so reaches the
register-staged ones.

COMPLETENESS: a census entry that is neither replayed nor exempt (the fused Cin = 1 / Cout = 1 entry points, each geometry mapped to the
test that checks it there) fails as a new launch without a value test.  The loader / consumer kernels size their persistent grid from
VIAI_DMA_GRID once per process: their launches are replayed once more in a child process with a grid of 61 blocks.
"""
import ctypes as C
import importlib.util
import json
import os
import subprocess
import sys
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# entry point -> {role: index of the argument after the descriptor}; pointer roles are recorded as set / NULL, the others by value
ROLES = {
    "viai_conv2d_fwd": {"x2": 1, "bias": 3, "stat": 5, "act": 6},
    "viai_conv2d_fwd_amax": {"x2": 1, "bias": 3, "stat": 5, "act": 6, "xa": 7},
    "viai_conv2d_fwd_p16": {"bias": 2, "stat": 4, "act": 5, "xa": 6},
    "viai_conv2d_dgrad": {"dx2": 3},
    "viai_conv2d_dgrad_f16": {"dx2": 3, "dya": 4},
    "viai_conv2d_dgrad_f16_p16": {"dx2": 3, "dya": 4},
    "viai_conv2d_wgrad": {"x2": 1, "db": 5, "acc": 6},
    "viai_conv2d_wgrad_f16": {"x2": 1, "db": 5, "acc": 6, "dya": 7, "xa": 8},
    "viai_conv2d_wgrad_f16_p16": {"x2": 1, "db": 5, "acc": 6, "dya": 7, "xa": 8, "flags": 9},
}
VALUE_ROLES = ("act", "acc", "flags")
# weight packing at a descriptor: checked wherever a replay packs with the same entry point at the same descriptor
PACKS = {"viai_conv2d_pack_fwd": "fwd", "viai_conv2d_pack_dgrad": "dgrad", "viai_conv2d_pack_dgrad_f16": "dgrad_f16"}
# the loader / consumer families whose persistent grid is VIAI_DMA_GRID (csrc/conv_halo_dma.hip viai_dma_grid)
DMA_GRID_FAMILIES = ("halo_wide256_f16x2", "halo_wide_s2_f16x2", "lin_dma_f16x2")

# Bounds, from the worst error measured on the MI355X over both censuses (139 replays, grid 256 and 61), at most ~3x it:
#   y 7.0e-7 (fwd_p16 1024x7x7 512->512, lin_dma), dx 7.5e-7 and tile 7.6e-7 (dgrad_f16_p16 16x64x32 256->512, halo_wide256),
#   dw 1.04e-6 and tap 1.1e-6 (wgrad_f16_p16 16x256x256 32->32 T), BatchNorm mean 2.8e-9 (of max |y|) and variance 1.25e-7,
#   adjointness 2.5e-10 (of |y| |gy|).  (The project's full-size bounds were 3e-6 / 3e-5 tile / 5e-6 tap / 1e-5 statistics.)
TOL = {"y": 2e-6, "dx": 2e-6, "dw": 3e-6, "db": 3e-6, "tile": 2.3e-6, "tap": 3.3e-6, "mean": 1e-8, "var": 4e-7, "adj": 7.5e-10}
# Weight gradients summed over more than 2^20 output pixels (the vision branch: 1024 frames) carry fp32 accumulation error that grows like
# sqrt(M): measured 2.2e-6 at M = 0.8 M (wgrad_patch 1024x28x28), 4.5e-6 at 3.2 M (wgrad_patch64 1024x56x56), 9.3e-6 / tap 1.1e-5 at
# 12.8 M (wgrad_stem 1024x224x224).  Their dw / tap bounds are scaled by 2 sqrt(M / 2^20); every launch at the audio sizes (M <= 2^20)
# keeps the plain bound.
DEEP_M = 1 << 20


def _bound(key, rec):
    b = TOL[key]
    if key in ("dw", "tap", "db"):
        from viai_amd import ops
        g = rec["desc"]
        d = ops.conv_desc(*g)
        M = g[0] * d["OH"] * d["OW"]
        if M > DEEP_M:
            b *= 2 * (M / DEEP_M) ** 0.5
    return b


SUBSET_N = 64          # batches above this (the vision branch's 1024 frames): y and dx on the first and last 4 images + adjointness

# The fused entry points are not replayed here: each (entry family, geometry) maps to the test that checks it at that geometry, and
# test_census_is_complete checks that the geometry is in that test's parameter list.
#   Cin = 1 conv + BatchNorm (viai_conv2d_cin1_bn_*): (N, H, W, Cout, kernel, stride, padding)
#   (conv + BatchNorm + act) -> Cout = 1 conv (viai_pair_cout1_*): (N, H, W, C of the pair's middle tensor, transposed)
CIN1_TEST = "tests/test_kernels_gpu.py::test_cin1_conv_bn_layer_without_the_stored_preactivation"
PAIR_TEST = "tests/test_kernels_gpu.py::test_fused_bn_cout1_pair_matches_the_two_layers"
EXEMPT = {
    ("viai_conv2d_cin1_bn", (16, 256, 256, 32, (3, 3), (2, 2), (1, 1))): CIN1_TEST,     # E.conv1
    ("viai_conv2d_cin1_bn", (16, 256, 256, 64, (1, 4), (1, 2), (0, 1))): CIN1_TEST,     # D.conv1 (and scale 0 of the 3-scale D)
    ("viai_conv2d_cin1_bn", (16, 128, 128, 64, (1, 4), (1, 2), (0, 1))): CIN1_TEST,     # D.conv1 of scale 1
    ("viai_conv2d_cin1_bn", (16, 64, 64, 64, (1, 4), (1, 2), (0, 1))): CIN1_TEST,       # D.conv1 of scale 2
    ("viai_pair_cout1", (16, 256, 256, 32, 1)): PAIR_TEST,                               # G.conv6_1 -> conv6_2
    ("viai_pair_cout1", (16, 64, 32, 512, 0)): PAIR_TEST,                                # D.conv3 -> conv4
    ("viai_pair_cout1", (16, 32, 16, 512, 0)): PAIR_TEST,                                # ... of scale 1 (scale 2 runs the two layers)
}


def _st():
    return torch.cuda.current_stream().cuda_stream


def _desc_tuple(d):
    from viai_amd._lib import Conv2dDesc
    return tuple(int(getattr(d, n)) for n, _ in Conv2dDesc._fields_)


def _fused_key(entry, desc):
    N, IH, IW, C1, C2, Co, kh, kw, sh, sw, ph, pw, tr = desc[:13]
    if entry.startswith("viai_conv2d_cin1_bn"):
        return "viai_conv2d_cin1_bn", (N, IH, IW, Co, (kh, kw), (sh, sw), (ph, pw))
    if entry.startswith("viai_pair_cout1"):
        return "viai_pair_cout1", (N, IH, IW, C1, tr)
    return None


# ---------------------------------------------------------------------------------------------------------------------------- census
def run_census(model, steps=1, run=None):
    """launch records of `steps` calls of `run(i)` (default: model.optimize_parameters): a list of dicts, deduplicated, values only"""
    run = model.optimize_parameters if run is None else run
    from viai_amd import _lib
    lib = _lib.load()
    names = [n for n, (_r, at) in _lib.SIGNATURES.items()
             if at and at[0] is _lib._CP and at[-1] is C.c_void_p and hasattr(lib, n)]
    buf = C.create_string_buffer(64)
    seen = {}
    orig = {}

    def wrap(name, fn):
        roles = ROLES.get(name, {})

        def spy(*args):
            r = fn(*args)
            d = getattr(args[0], "_obj", None) if args else None
            if not isinstance(d, _lib.Conv2dDesc):
                return r
            nl = lib.viai_conv2d_last_kernel(buf, 64)
            fam = buf.value.decode()
            rest = args[1:]
            opts = tuple(sorted((k, int(rest[i] or 0) if k in VALUE_ROLES else bool(rest[i])) for k, i in roles.items()))
            key = (name, _desc_tuple(d), fam, opts)
            if key not in seen:
                seen[key] = {"entry": name, "desc": list(key[1]), "family": fam, "launches": nl, "opts": dict(opts), "count": 0}
            seen[key]["count"] += 1
            return r
        return spy

    try:
        for n in names:
            fn = getattr(lib, n)
            orig[n] = fn
            setattr(lib, n, wrap(n, fn))
        for i in range(steps):
            run(i)
        torch.cuda.synchronize()
    finally:
        for n, fn in orig.items():
            setattr(lib, n, fn)
    return list(seen.values())


def _census_cfg1():
    from oracle import viai_oracle as O
    from viai_amd import synth
    from viai_amd.model import AudioModel, StepConfig
    hp = StepConfig()
    hp.cin_channels, hp.max_mel_lengths = 256, 256
    m = AudioModel(hp, device="cuda")
    m.load_states(O.encoder_state(), O.decoder_state(), O.disc_state())
    m.set_inputs(synth.mel_batch(16, 256, 256, "census.s", 0).cuda(), synth.time_mask(16, 256, "census.mask", 0).cuda())
    try:
        return run_census(m)
    finally:
        del m
        torch.cuda.empty_cache()


def _census_cfg3():
    from oracle import viai_oracle as O
    from viai_amd import synth
    from viai_amd.model import AudioModel, StepConfig
    B, NF = 16, 64
    hp = StepConfig()
    hp.cin_channels, hp.max_mel_lengths = 256, 256
    hp.use_video, hp.num_D, hp.lambda_contrast = True, 3, 0.1
    m = AudioModel(hp, device="cuda")
    m.load_states(O.encoder_state(), O.decoder_variant_state("image"), O.msd_state(3), O.image_embedding2_state())
    m.set_inputs(synth.mel_batch(B, 256, 256, "census.av.s", 0).cuda(), synth.time_mask(B, 256, "census.av.mask", 0).cuda(),
                 video=synth.uniform("census.av.video", (B, NF, 3, 224, 224), -1, 1).cuda(),
                 flow=synth.uniform("census.av.flow", (B, NF, 2, 224, 224), -1, 1).cuda())
    try:
        return run_census(m)
    finally:
        m.close()
        del m
        torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------------------- replay
def _to_p16(t):
    """fp32 NHWC tensor -> (P16 tensor, bound slot, decoded fp32 tensor): the forward BatchNorm producer with identity coefficients, whose
    bound is the step's rule sqrt(M - 1) (gamma = 1, beta = 0), not the tensor's maximum"""
    from viai_amd import _lib
    lib = _lib.load()
    Cc = t.shape[-1]
    M = t.numel() // Cc
    one, zero = torch.ones(Cc, device="cuda"), torch.zeros(Cc, device="cuda")
    p, am = torch.empty_like(t), torch.zeros(1, device="cuda")
    _lib.check(lib.viai_bn_act_fwd_p16(t.data_ptr(), one.data_ptr(), zero.data_ptr(), one.data_ptr(), zero.data_ptr(), M, p.data_ptr(), M, Cc, 0, 0.2,
                                       am.data_ptr(), _st()), "viai_bn_act_fwd_p16")
    dec = torch.empty_like(t)
    _lib.check(lib.viai_p16_decode(p.data_ptr(), dec.data_ptr(), M, Cc, am.data_ptr(), _st()), "viai_p16_decode")
    return p, am, dec


def _amax(*ts):
    return torch.stack([t.abs().max() for t in ts if t is not None]).max().reshape(1).contiguous()


class _Geom:
    def __init__(self, desc):
        (self.N, self.IH, self.IW, self.C1, self.C2, self.Co, self.kh, self.kw, self.sh, self.sw, self.ph, self.pw, self.tr,
         self.dh, self.dw, self.ph2, self.pw2) = desc
        from viai_amd import ops
        self.d = ops.conv_desc(*desc)
        self.OH, self.OW = self.d["OH"], self.d["OW"]
        self.Cin = self.C1 + self.C2
        self.frames = self.C2 == 0 and 1 < self.C1 < 4          # the ResNet stem: 2 / 3-channel frames stored at channel stride 4
        self.pb = self.ph if self.ph2 < 0 else self.ph2
        self.pr = self.pw if self.pw2 < 0 else self.pw2
        self.wshape = (self.Cin, self.Co, self.kh, self.kw) if self.tr else (self.Co, self.Cin, self.kh, self.kw)

    def short(self):
        s = "%dx%dx%d %d%s->%d k%dx%d s%d,%d p%d,%d%s" % (self.N, self.IH, self.IW, self.C1, "+%d" % self.C2 if self.C2 else "", self.Co,
                                                        self.kh, self.kw, self.sh, self.sw, self.ph, self.pw, " T" if self.tr else "")
        if self.dh != 1 or self.dw != 1:
            s += " d%d,%d" % (self.dh, self.dw)
        if self.ph2 >= 0 or self.pw2 >= 0:
            s += " p2 %d,%d" % (self.pb, self.pr)
        return s

    # fp64 truth on NCHW tensors (CPU): the layer as torch.nn.functional defines it, padding made explicit where it is asymmetric
    def _args(self):
        asym = (self.pb, self.pr) != (self.ph, self.pw)
        if asym and self.tr:
            raise NotImplementedError("asymmetric padding of a transposed conv")
        pad = (0, 0) if asym else (self.ph, self.pw)
        opad = (0, 0)
        if self.tr:
            opad = (self.OH - ((self.IH - 1) * self.sh - 2 * self.ph + self.dh * (self.kh - 1) + 1),
                    self.OW - ((self.IW - 1) * self.sw - 2 * self.pw + self.dw * (self.kw - 1) + 1))
        return asym, pad, opad

    def _padx(self, x):
        return torch.nn.functional.pad(x, (self.pw, self.pr, self.ph, self.pb))

    def fwd64(self, x, w):
        asym, pad, opad = self._args()
        if asym:
            x = self._padx(x)
        return torch.ops.aten.convolution(x, w, None, [self.sh, self.sw], list(pad), [self.dh, self.dw], bool(self.tr), list(opad), 1)

    def bwd64(self, x, w, dy, need_x, need_w):
        """(dx, dw) of <conv(x, w), dy>; x may be a meta-shaped stand-in when only dx is wanted"""
        asym, pad, opad = self._args()
        if asym:
            x = self._padx(x)
        dx, dw, _ = torch.ops.aten.convolution_backward(dy, x, w, None, [self.sh, self.sw], list(pad), [self.dh, self.dw], bool(self.tr),
                                                        list(opad), 1, [need_x, need_w, False])
        if need_x and asym:
            dx = dx[:, :, self.ph:self.ph + self.IH, self.pw:self.pw + self.IW]
        return dx, dw


def _nchw64(t, c=None):
    """NHWC (cuda, fp32) -> NCHW fp64 CPU, first c channels"""
    t = t if c is None else t[..., :c]
    return t.permute(0, 3, 1, 2).double().cpu()


def _relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-300)).item()


def _worst_tile(a, b, th=8, tw=16):
    """largest relative error of any th x tw output tile of an NCHW tensor (tests/test_fullsize_gpu.py)"""
    N, Cc, H, W = a.shape
    if H % th or W % tw:
        return _relerr(a, b)
    d = (a - b).pow(2).reshape(N, Cc, H // th, th, W // tw, tw).sum(dim=(1, 3, 5))
    r = b.pow(2).reshape(N, Cc, H // th, th, W // tw, tw).sum(dim=(1, 3, 5))
    return float((d / (r + 1e-300)).sqrt().max())


def _act64(y, act):
    if act == 1:
        return y.clamp_min(0)
    if act == 2:
        return torch.nn.functional.leaky_relu(y, 0.2)
    if act == 3:
        return torch.sigmoid(y)
    return y


def _images(n):
    """the images checked in full: all of them, or the first and last 4 (the first and the last persistent work items) of a large batch"""
    return list(range(n)) if n <= SUBSET_N else list(range(4)) + list(range(n - 4, n))


def _wgrad64(g, x64_of, dy64_of, w64):
    """fp64 weight gradient over the whole batch, in chunks of images (bounded host memory)"""
    acc = None
    for i in range(0, g.N, 32):
        sl = slice(i, min(g.N, i + 32))
        _, dw = g.bwd64(x64_of(sl), w64, dy64_of(sl), False, True)
        acc = dw if acc is None else acc + dw
    return acc


def replay(rec, gen, worst_tile=None, keep=None):
    """one census launch again on fresh operands: (family seen, {quantity: error}); raises on a library error.
    `worst_tile`: the tile error to use instead of _worst_tile (tests/test_inference_launches_gpu.py: clipped tiles); `keep`: a dict that
    receives the forward's fp64 operands and results (x, w, bias, act, y, truth), for a second opinion on the same operands"""
    worst_tile = _worst_tile if worst_tile is None else worst_tile
    from oracle import viai_oracle as O
    from viai_amd import _lib, ops
    lib = _lib.load()
    entry, opts = rec["entry"], rec["opts"]
    g = _Geom(tuple(rec["desc"]))
    d, st = g.d, _st()
    dev = "cuda"
    errs = {}
    fam = C.create_string_buffer(64)
    w = O.cf_std("launch.w.%d.%d.%d.%d" % (g.Cin, g.Co, g.kh, g.kw), g.wshape, 1.0 / (g.Cin * g.kh * g.kw) ** 0.5).to(dev)
    w64 = w.double().cpu()
    imgs = _images(g.N)
    subset = len(imgs) < g.N

    def uni(shape, scale=1.0):
        return (torch.rand(shape, device=dev, generator=gen) * 2 - 1) * scale

    def make_x(p16):
        """(x as the kernel reads it, its amax slot or None, x as fp32 values on C1 channels, x2 or None)"""
        if g.frames:
            fr = uni((g.N, g.C1, g.IH, g.IW))
            x = ops.frames_to_nhwc4(fr)
            return x, x._viai_amax, x, None
        x = uni((g.N, g.IH, g.IW, g.C1))
        x2 = uni((g.N, g.IH, g.IW, g.C2)) if g.C2 else None
        if p16:
            xp, am, dec = _to_p16(x)
            return xp, am, dec, None
        return x, None, x, x2

    def make_dy(p16):
        dy = uni((g.N, g.OH, g.OW, g.Co), 1e-3)
        if p16:
            return _to_p16(dy)
        return dy, None, dy

    def x64_cat(xv, x2, sl):
        a = _nchw64(xv[sl], g.C1)
        return torch.cat((a, _nchw64(x2[sl])), 1) if x2 is not None else a

    def tag():
        lib.viai_conv2d_last_kernel(fam, 64)
        return fam.value.decode()

    if entry.startswith("viai_conv2d_fwd"):
        p16 = entry == "viai_conv2d_fwd_p16"
        x, xa, xv, x2 = make_x(p16)
        if entry == "viai_conv2d_fwd_amax" and opts["xa"] and xa is None:
            xa = _amax(xv, x2)
        wp = torch.empty(d["packed"], device=dev)
        _lib.check(lib.viai_conv2d_pack_fwd(d["ref"], w.data_ptr(), wp.data_ptr(), st), "pack_fwd")
        bias = uni((g.Co,), 0.1) if opts["bias"] else None
        y = torch.empty(g.N, g.OH, g.OW, g.Co, device=dev)
        M = g.N * g.OH * g.OW
        stat = torch.empty(2 * g.Co * max(d["nblk"], -(-M // 128)), device=dev) if opts["stat"] else None
        act = opts["act"]
        if p16:
            _lib.check(lib.viai_conv2d_fwd_p16(d["ref"], x.data_ptr(), wp.data_ptr(), ops._ptr(bias), y.data_ptr(), ops._ptr(stat), act, xa.data_ptr(), st), entry)
        elif entry == "viai_conv2d_fwd_amax":
            _lib.check(lib.viai_conv2d_fwd_amax(d["ref"], x.data_ptr(), ops._ptr(x2), wp.data_ptr(), ops._ptr(bias), y.data_ptr(), ops._ptr(stat), act,
                                                ops._ptr(xa) if opts["xa"] else 0, st), entry)
        else:
            _lib.check(lib.viai_conv2d_fwd(d["ref"], x.data_ptr(), ops._ptr(x2), wp.data_ptr(), ops._ptr(bias), y.data_ptr(), ops._ptr(stat), act, st), entry)
        seen = tag()
        if stat is not None:
            coef = torch.empty(4, g.Co, device=dev)
            cfg = {"momentum": 0.1, "eps": ops.BN_EPS}
            lin = p16 and bool(ops.p16_mask(d) & ops.P16_OK_FWD_LIN)
            ops._bn_finalize(lib, d, stat, M, g.Co, torch.ones(g.Co, device=dev), torch.zeros(g.Co, device=dev), None, None, None, cfg, coef, st, lin=lin)
            yd = y.view(-1, g.Co).double()
            mu, var = yd.mean(0), yd.var(0, unbiased=False)
            var_k = coef[1].double().pow(-2) - ops.BN_EPS
            errs["mean"] = ((coef[0].double() - mu).abs().max() / yd.abs().max()).item()
            errs["var"] = ((var_k - var).abs() / var).max().item()
        torch.cuda.synchronize()
        ytrue = _act64(g.fwd64(x64_cat(xv, x2, imgs), w64) + (bias.double().cpu().view(1, -1, 1, 1) if bias is not None else 0), act)
        yk = _nchw64(y[imgs])
        errs["y"] = _relerr(yk, ytrue)
        errs["tile"] = worst_tile(yk, ytrue)
        if keep is not None:
            keep.update(x=x64_cat(xv, x2, imgs), w=w64, bias=bias.double().cpu() if bias is not None else None, act=act, y=yk, truth=ytrue)
        if subset and not g.frames and act == 0 and bias is None:
            # <y, gy> = <x, dgrad(gy)> over the whole batch, the data gradient from the plain kernel of the same layer
            gy = uni(tuple(y.shape))
            wpd = torch.empty(d["packed"], device=dev)
            _lib.check(lib.viai_conv2d_pack_dgrad(d["ref"], w.data_ptr(), wpd.data_ptr(), st), "pack_dgrad")
            dx = torch.empty(g.N, g.IH, g.IW, g.C1, device=dev)
            dx2 = torch.empty(g.N, g.IH, g.IW, g.C2, device=dev) if g.C2 else None
            _lib.check(lib.viai_conv2d_dgrad(d["ref"], gy.data_ptr(), wpd.data_ptr(), dx.data_ptr(), ops._ptr(dx2), st), "dgrad (adjoint)")
            lhs = (y.double() * gy.double()).sum().item()
            rhs = (xv.double() * dx.double()).sum().item() + ((x2.double() * dx2.double()).sum().item() if dx2 is not None else 0.0)
            errs["adj"] = abs(lhs - rhs) / (y.double().norm() * gy.double().norm()).item()
        return seen, errs

    if entry.startswith("viai_conv2d_dgrad"):
        p16 = entry.endswith("_p16")
        dy, am, dyv = make_dy(p16)
        if entry == "viai_conv2d_dgrad_f16":
            am = _amax(dy)
        form = "viai_conv2d_pack_dgrad" if entry == "viai_conv2d_dgrad" else "viai_conv2d_pack_dgrad_f16"
        wp = torch.empty(d["packed"], device=dev)
        _lib.check(getattr(lib, form)(d["ref"], w.data_ptr(), wp.data_ptr(), st), form)
        dx = torch.empty(g.N, g.IH, g.IW, g.C1, device=dev)
        dx2 = torch.empty(g.N, g.IH, g.IW, g.C2, device=dev) if opts["dx2"] else None
        if entry == "viai_conv2d_dgrad":
            _lib.check(lib.viai_conv2d_dgrad(d["ref"], dy.data_ptr(), wp.data_ptr(), dx.data_ptr(), ops._ptr(dx2), st), entry)
        else:
            _lib.check(getattr(lib, entry)(d["ref"], dy.data_ptr(), wp.data_ptr(), dx.data_ptr(), ops._ptr(dx2), am.data_ptr(), st), entry)
        seen = tag()
        torch.cuda.synchronize()
        xshape = torch.empty(len(imgs), g.Cin, g.IH, g.IW, dtype=torch.float64)
        dtrue, _ = g.bwd64(xshape, w64, _nchw64(dyv[imgs]), True, False)
        dk = _nchw64(dx[imgs])
        if dx2 is not None:
            dk = torch.cat((dk, _nchw64(dx2[imgs])), 1)
        errs["dx"] = _relerr(dk, dtrue)
        errs["tile"] = worst_tile(dk, dtrue)
        if subset:
            # <x, dx> = <fwd(x), dy> over the whole batch, the forward from the plain kernel of the same layer
            x = uni((g.N, g.IH, g.IW, g.C1))
            x2 = uni((g.N, g.IH, g.IW, g.C2)) if g.C2 else None
            wpf = torch.empty(d["packed"], device=dev)
            _lib.check(lib.viai_conv2d_pack_fwd(d["ref"], w.data_ptr(), wpf.data_ptr(), st), "pack_fwd")
            y = torch.empty(g.N, g.OH, g.OW, g.Co, device=dev)
            _lib.check(lib.viai_conv2d_fwd(d["ref"], x.data_ptr(), ops._ptr(x2), wpf.data_ptr(), 0, y.data_ptr(), 0, 0, st), "fwd (adjoint)")
            lhs = (x.double() * dx.double()).sum().item() + ((x2.double() * dx2.double()).sum().item() if x2 is not None else 0.0)
            rhs = (y.double() * dyv.double()).sum().item()
            errs["adj"] = abs(lhs - rhs) / (y.double().norm() * dyv.double().norm()).item()
        return seen, errs

    # weight gradients
    flags = opts.get("flags", 0)
    x, xa, xv, x2 = make_x(bool(flags & 2))
    dy, dya, dyv = make_dy(bool(flags & 1))
    if entry != "viai_conv2d_wgrad" and opts["dya"] and dya is None:
        dya = _amax(dy)
    if entry != "viai_conv2d_wgrad" and opts["xa"] and xa is None:
        xa = _amax(xv, x2)
    dtrue = _wgrad64(g, lambda sl: x64_cat(xv, x2, sl), lambda sl: _nchw64(dyv[sl]), w64)
    dw0 = (torch.rand(g.wshape, generator=torch.Generator().manual_seed(3), dtype=torch.float64) * 2 - 1) * dtrue.abs().max()
    dw = dw0.float().to(dev) if opts["acc"] else torch.empty(g.wshape, device=dev)
    db = torch.zeros(g.Co, device=dev) if opts["db"] else None
    db0 = db.clone() if db is not None else None
    ws = torch.empty(max(1, d["ws_floats"]), device=dev)
    if entry == "viai_conv2d_wgrad":
        _lib.check(lib.viai_conv2d_wgrad(d["ref"], x.data_ptr(), ops._ptr(x2), dy.data_ptr(), ws.data_ptr(), dw.data_ptr(), ops._ptr(db), opts["acc"], st), entry)
    elif entry == "viai_conv2d_wgrad_f16":
        _lib.check(lib.viai_conv2d_wgrad_f16(d["ref"], x.data_ptr(), ops._ptr(x2), dy.data_ptr(), ws.data_ptr(), dw.data_ptr(), ops._ptr(db), opts["acc"],
                                             ops._ptr(dya) if opts["dya"] else 0, ops._ptr(xa) if opts["xa"] else 0, st), entry)
    else:
        _lib.check(lib.viai_conv2d_wgrad_f16_p16(d["ref"], x.data_ptr(), ops._ptr(x2), dy.data_ptr(), ws.data_ptr(), dw.data_ptr(), ops._ptr(db), opts["acc"],
                                                 ops._ptr(dya) if opts["dya"] else 0, ops._ptr(xa) if opts["xa"] else 0, flags, st), entry)
    seen = tag()
    torch.cuda.synchronize()
    dk = dw.double().cpu() - (dw0.float().double() if opts["acc"] else 0)
    errs["dw"] = _relerr(dk, dtrue)
    kk = dk.shape[2] * dk.shape[3]
    errs["tap"] = max(_relerr(dk[:, :, t // dk.shape[3], t % dk.shape[3]], dtrue[:, :, t // dk.shape[3], t % dk.shape[3]]) for t in range(kk))
    if db is not None:
        errs["db"] = _relerr(db.double() - db0.double(), dyv.double().sum(dim=(0, 1, 2)))
    return seen, errs


def _replayable(rec):
    return rec["entry"] in ROLES


# (pass, form) of viai_conv2d_route for the launch entry points (include/viai_hip.h: VIAI_FORM_*)
ROUTE_OF = {"viai_conv2d_fwd": (0, 0), "viai_conv2d_fwd_amax": (0, 1), "viai_conv2d_fwd_p16": (0, 2),
            "viai_conv2d_dgrad": (1, 0), "viai_conv2d_dgrad_f16": (1, 1), "viai_conv2d_dgrad_f16_p16": (1, 2),
            "viai_conv2d_wgrad": (2, 0), "viai_conv2d_wgrad_f16": (2, 1), "viai_conv2d_wgrad_f16_p16": (2, 2)}


def _route(lib, rec):
    """(family, launches) viai_conv2d_route predicts for a census record"""
    from viai_amd._lib import Conv2dDesc
    p, f = ROUTE_OF[rec["entry"]]
    if rec["entry"] == "viai_conv2d_wgrad_f16_p16":
        f = (f | (rec["opts"]["flags"] << 2)) if rec["opts"]["flags"] else 1          # (no flags: the plain f16x2 form)
    buf = C.create_string_buffer(64)
    d = Conv2dDesc(*rec["desc"])
    n = lib.viai_conv2d_route(C.byref(d), p, f, buf, 64)
    return buf.value.decode(), n


def replay_all(records, label, out=print):
    """replay every record, collecting (row, failure or None); one table printed"""
    gen = torch.Generator(device="cuda").manual_seed(20261016)
    nthreads = torch.get_num_threads()
    torch.set_num_threads(min(16, nthreads))
    rows, bad = [], []
    try:
        for rec in sorted(records, key=lambda r: (r["entry"], r["desc"])):
            if not _replayable(rec):
                continue
            g = _Geom(tuple(rec["desc"]))
            t0 = time.time()
            try:
                seen, errs = replay(rec, gen)
                msg = None
                if seen != rec["family"]:
                    msg = "family %s, the step ran %s" % (seen, rec["family"])
                over = [k for k, v in errs.items() if not v <= _bound(k, rec)]
                if over:
                    msg = (msg + "; " if msg else "") + "over the bound: " + ", ".join(over)
            except Exception as e:          # (a library error is a finding of this launch: report it with the others)
                seen, errs, msg = "?", {}, "%s: %s" % (type(e).__name__, e)
            opt = " ".join("%s=%d" % (k, v) for k, v in sorted(rec["opts"].items()) if v)
            row = "%-26s %-40s %-24s %-28s %s  (%.1fs)" % (rec["entry"][12:], g.short(), rec["family"], opt,
                                                         " ".join("%s %.2e" % kv for kv in sorted(errs.items())), time.time() - t0)
            rows.append(row)
            out(("FAIL " if msg else "ok   ") + row + ("  <-- " + msg if msg else ""))
            if msg:
                bad.append("%s %s [%s]: %s" % (rec["entry"], g.short(), rec["family"], msg))
            torch.cuda.empty_cache()
    finally:
        torch.set_num_threads(nthreads)
    return rows, bad


# ---------------------------------------------------------------------------------------------------------------------------- tests
@pytest.fixture(scope="module")
def census(tmp_path_factory):
    t0 = time.time()
    c = {"cfg1": _census_cfg1(), "cfg3": _census_cfg3()}
    path = tmp_path_factory.mktemp("census") / "census.json"
    path.write_text(json.dumps(c))
    print("\ncensus: %d + %d distinct launches in %.1f s" % (len(c["cfg1"]), len(c["cfg3"]), time.time() - t0))
    for k, recs in c.items():
        for r in sorted(recs, key=lambda r: (r["entry"], r["desc"])):
            g = _Geom(tuple(r["desc"]))
            print("  %s %-30s %-40s %-24s %s x%d" % (k, r["entry"][5:], g.short(), r["family"],
                                                   " ".join("%s=%d" % kv for kv in sorted(r["opts"].items()) if kv[1]), r["count"]))
    return c, path


def _load_test_module(name):
    spec = importlib.util.spec_from_file_location("_launch_census_" + name, os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_census_is_complete(census):
    """the census itself is sane, every hand-written full-size layer of tests/test_fullsize_gpu.py still occurs in the step, and every
    launch is either replayed here or checked at its geometry by the test its exemption names"""
    c, _ = census
    allrec = c["cfg1"] + c["cfg3"]
    assert c["cfg1"] and c["cfg3"]
    assert any(r["entry"] == "viai_conv2d_fwd_p16" for r in c["cfg1"])
    assert any(r["entry"] == "viai_conv2d_fwd_p16" for r in c["cfg3"])
    from viai_amd import _lib
    lib = _lib.load()
    routed = [r for r in allrec if r["entry"] in ROUTE_OF]
    assert routed
    off = ["%s %s: launched %s x%d, route %s x%d" % ((r["entry"], _Geom(tuple(r["desc"])).short(), r["family"], r["launches"]) + _route(lib, r))
           for r in routed if _route(lib, r) != (r["family"], r["launches"])]
    assert not off, "viai_conv2d_route disagrees with the launch:\n  " + "\n  ".join(off)
    shapes = {(r["desc"][0], r["desc"][1], r["desc"][2], r["desc"][3] + r["desc"][4], r["desc"][5], (r["desc"][6], r["desc"][7]),
               (r["desc"][8], r["desc"][9]), (r["desc"][10], r["desc"][11]), bool(r["desc"][12])) for r in c["cfg1"]}
    fs = _load_test_module("test_fullsize_gpu")
    stale = []
    for case in fs.FULL_LAYERS + fs.MORE_LAYERS:
        name, N, H, W, C1, Co, k, s, p, tr = case[:10]
        Cin = C1 + (case[10] if len(case) > 10 else 0)
        if ((N, H, W, Cin, Co, tuple(k), tuple(s), tuple(p), bool(tr)) in shapes) == (name in fs.NOT_IN_STEP):
            stale.append(name)
    assert not stale, "tests/test_fullsize_gpu.py: layer lists (or NOT_IN_STEP) out of date with the step: %s" % stale

    kt = _load_test_module("test_kernels_gpu")
    listed = {CIN1_TEST: {(g[0], g[1], g[2], g[3], tuple(g[4]), tuple(g[5]), tuple(g[6])) for g in kt.CIN1_GEOMS},
              PAIR_TEST: {(v[0], v[3], v[4], v[2], int(n.startswith("G."))) for n, v in kt.PAIR_CASES.items()}}
    for (fam, geom), test in EXEMPT.items():
        assert geom in listed[test], "exemption %s %s names %s, which does not run that geometry" % (fam, geom, test)
    missing = []
    for r in allrec:
        if _replayable(r) or r["entry"] in PACKS:
            continue
        key = _fused_key(r["entry"], r["desc"])
        if key is None or key not in EXEMPT:
            missing.append("%s %s" % (r["entry"], _Geom(tuple(r["desc"])).short()))
    # weight packing at a descriptor counts as checked where a replayed launch packs with that entry point at that descriptor
    packed = set()
    for r in allrec:
        e = r["entry"]
        if e in ("viai_conv2d_fwd", "viai_conv2d_fwd_amax", "viai_conv2d_fwd_p16"):
            packed.add(("viai_conv2d_pack_fwd", tuple(r["desc"])))
        elif e == "viai_conv2d_dgrad":
            packed.add(("viai_conv2d_pack_dgrad", tuple(r["desc"])))
        elif e in ("viai_conv2d_dgrad_f16", "viai_conv2d_dgrad_f16_p16"):
            packed.add(("viai_conv2d_pack_dgrad_f16", tuple(r["desc"])))
        elif _fused_key(e, r["desc"]) in EXEMPT:                               # (the fused layers' tests pack their weights as the step does)
            packed.update((pk, tuple(r["desc"])) for pk in ("viai_conv2d_pack_fwd", "viai_conv2d_pack_dgrad"))
    for r in allrec:
        if r["entry"] in PACKS and (r["entry"], tuple(r["desc"])) not in packed:
            missing.append("%s %s" % (r["entry"], _Geom(tuple(r["desc"])).short()))
    assert not missing, "new launch without a value test:\n  " + "\n  ".join(sorted(set(missing)))


def _replay_test(records, label):
    t0 = time.time()
    print("\nreplay of the %s step's launches against fp64:" % label)
    rows, bad = replay_all(records, label)
    print("%d launches in %.1f s" % (len(rows), time.time() - t0))
    assert rows
    assert not bad, "%d of %d launches of the %s step off:\n  " % (len(bad), len(rows), label) + "\n  ".join(bad)


def test_audio_step_launches_against_fp64(census):
    """BASELINE.json configs[1]: every distinct conv launch of the 16 x 256 x 256 step"""
    c, _ = census
    recs = [r for r in c["cfg1"] if _replayable(r)]
    assert any(r["family"] == "halo_wide256_f16x2" and r["entry"] == "viai_conv2d_fwd_p16" and r["desc"][:6] == [16, 64, 32, 256, 0, 512] for r in recs)
    assert any(r["entry"] == "viai_conv2d_wgrad_f16_p16" and r["opts"]["flags"] == 3 for r in recs)
    _replay_test(recs, "audio (configs[1])")


def test_vision_infused_step_launches_against_fp64(census):
    """BASELINE.json configs[3] on one device: the launches that step adds (ResNet-18 over 1024 + 1024 frames, two smaller D scales, the
    image-conditioned decoder)"""
    c, _ = census
    have = {(r["entry"], tuple(r["desc"]), r["family"], tuple(sorted(r["opts"].items()))) for r in c["cfg1"]}
    recs = [r for r in c["cfg3"] if _replayable(r) and (r["entry"], tuple(r["desc"]), r["family"], tuple(sorted(r["opts"].items()))) not in have]
    assert any(r["family"] == "lin_dma_f16x2" and r["desc"][0] == 1024 for r in recs)
    _replay_test(recs, "vision-infused (configs[3])")


def test_loader_consumer_launches_on_a_61_block_grid(census):
    """VIAI_DMA_GRID=61: many work items per block, in counts that do not divide evenly -- a fresh process (the grid is read once)"""
    c, path = census
    n = sum(1 for k in c for r in c[k] if _replayable(r) and r["family"] in DMA_GRID_FAMILIES)
    assert n > 0
    env = dict(os.environ, VIAI_DMA_GRID="61", PYTHONPATH=os.pathsep.join([ROOT] + [p for p in [os.environ.get("PYTHONPATH")] if p]))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--replay", str(path)], env=env, cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1200)
    print(r.stdout[-20000:])
    assert r.returncode == 0, "replay on a 61-block grid failed (exit %d):\n%s" % (r.returncode, r.stdout[-6000:])


def _child_main(path):
    """the VIAI_DMA_GRID child: replay the loader / consumer launches of both censuses"""
    c = json.loads(open(path).read())
    seen, recs = set(), []
    for k in ("cfg1", "cfg3"):
        for r in c[k]:
            key = (r["entry"], tuple(r["desc"]), r["family"], tuple(sorted(r["opts"].items())))
            if _replayable(r) and r["family"] in DMA_GRID_FAMILIES and key not in seen:
                seen.add(key)
                recs.append(r)
    print("VIAI_DMA_GRID=%s: %d launches" % (os.environ.get("VIAI_DMA_GRID"), len(recs)))
    rows, bad = replay_all(recs, "grid 61")
    print("\n".join(bad))
    return 1 if bad or not rows else 0


if __name__ == "__main__":
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    if len(sys.argv) == 3 and sys.argv[1] == "--replay":
        sys.exit(_child_main(sys.argv[2]))
    sys.exit("usage: test_step_launches_gpu.py --replay CENSUS.json")
