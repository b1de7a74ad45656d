"""The conv dispatch table, pinned without a GPU.

tests/golden/conv_routes.json was recorded with tools/conv_routes.py from the library as it stood BEFORE the routes were gathered into
route_fwd / route_dgrad / route_wgrad (csrc/conv_api.hip): what every query answered and which (return code, launch count, kernel family)
each of the nine launch entry points tagged.  Its descriptors are
  * FULL_LAYERS + MORE_LAYERS of tests/test_fullsize_gpu.py (the layers of the audio step, configs[1]), and its discriminator layers again
    at half and quarter size (the two smaller scales of the vision-infused step, configs[3]),
  * the ResNet-18 convs over 1024 frames (7 x 7 stem, the 3 x 3 layers at 56 / 28 / 14 / 7 squared, the 1 x 1 stride-2 shortcuts),
  * sweep rows of tools/conv_routes.py chosen so that every (entry point, family), every P16 mask, every partial geometry and every
    triple of weight layouts occurs at least three times,
  * the Conv1d layers of a teacher-forced WaveNet step (tools/conv_routes.py wavenet_descs: 17-field descriptors, the k = 3 layer dilated
    and padded on the left only), recorded from the library with the gathered routes.
Here viai_conv2d_route and the queries must give the recorded answers.  Nothing is launched.

FAMILIES has 38 names: the 37 MFMA / halo / DMA / weight-gradient families plus "direct", the Cin = 1 / Cout = 1 streaming kernels.

What the recording cannot pin: a strided data gradient that runs class by class stopped, without a device, at the launch of its first
parity class, so the record holds that class's tile instance and a count of one.  The route names the LAST class (as the tag does after a
real call) and counts every live class; for those rows the test checks the arithmetic of the family and a count derived from the taps.
The table was put together without a run of the step census (run_census needs the GPU), so a descriptor of the image-conditioned
decoder may be missing here; tests/test_step_launches_gpu.py compares the route with every real launch of both steps.
"""
import ctypes as C
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = json.load(open(os.path.join(ROOT, "tests", "golden", "conv_routes.json")))
NO_DEVICE = 100          # hipErrorNoDevice: the recorded call chose its kernel and failed at the launch
FAMILIES = {"direct", "stem_f16x2", "igemm64x64_f32", "igemm128x128_f32", "igemm128x64_f32", "igemm128x32_f32",
            "igemm64x64_bf16x3", "igemm128x128_bf16x3", "igemm128x64_bf16x3", "igemm128x32_bf16x3",
            "igemm64x64_f16x2", "igemm128x128_f16x2", "igemm128x64_f16x2", "igemm128x32_f16x2", "igemm128x256_f16x2",
            "igemm_sk32x32_bf16x3", "igemm_sk32x32_f16x2", "halo_bf16x3", "halo_f16x2", "halo_c32_f16x2",
            "halo_wide32_f16x2", "halo_wide64_f16x2", "halo_wide128_f16x2", "halo_wide256_f16x2", "halo_wide_s2_f16x2", "lin_dma_f16x2",
            "dgrad_s2_bf16x3", "dgrad_s2_f16x2", "dgrad_s2_patch_f16x2",
            "wgrad_mfma_f32", "wgrad32_all_taps_f32", "wgrad_bf3_bf16x3", "wgrad_bf3_f16x2", "wgrad_stem_f16x2",
            "wgrad_patch_f16x2", "wgrad_patch64_f16x2", "wgrad_patch_narrow_f16x2", "wgrad_patch_s2_f16x2"}


def _tool():
    spec = importlib.util.spec_from_file_location("_conv_routes_tool", os.path.join(ROOT, "tools", "conv_routes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def lib():
    from viai_amd import _lib
    return _lib.load()


def _desc17(d):
    """the 17 descriptor fields of a row: 13 recorded fields mean no dilation and symmetric padding (tools/conv_routes.py desc17)"""
    return tuple(d) + (0, 0, -1, -1) if len(d) == 13 else tuple(d)


def _cin1_without_kernel(d):
    """Cin = 1 outside the streaming kernels' windows and 32 / 64 / 128 output channels: refused since ABI 18 (its entry points used to
    tag "direct" and fail, the weight gradient with a division by zero for Cout < 4)"""
    N, IH, IW, C1, C2, Co, kh, kw = d[:8]
    return C1 + C2 == 1 and not (Co in (32, 64, 128) and (kh, kw) in ((3, 3), (1, 1), (1, 3), (1, 4), (1, 6)))


def _live_classes(d):
    """parity classes of the data gradient that exist and have a tap: one launch each on the class-by-class kernels"""
    IH, IW, kh, kw, sh, sw, ph, pw = d[1], d[2], d[6], d[7], d[8], d[9], d[10], d[11]
    rows = {(r - ph) % sh for r in range(kh)} & set(range(min(sh, IH)))
    cols = {(s - pw) % sw for s in range(kw)} & set(range(min(sw, IW)))
    return len(rows) * len(cols)


def test_golden_table_reaches_every_family():
    fams = {x[2] for r in ROWS for x in r[12:21] if x[2]}
    assert len(FAMILIES) == 38 and len(ROWS) >= 150 and fams == FAMILIES, sorted(fams ^ FAMILIES)


def test_queries_answer_as_recorded(lib):
    from viai_amd._lib import Conv2dDesc, PackJob
    i1, i2 = C.c_int(), C.c_int()
    for r in ROWS:
        d = r[0]
        c = Conv2dDesc(*_desc17(d))
        rc = lib.viai_conv2d_stat_geom(C.byref(c), C.byref(i1), C.byref(i2))
        if _cin1_without_kernel(d):
            assert rc != 0 and lib.viai_conv2d_wgrad_ws_bytes(C.byref(c)) == 0, d
            continue
        assert [rc, i1.value, i2.value] == r[1], d
        assert [lib.viai_conv2d_stat_tiles(C.byref(c), C.byref(i1), C.byref(i2)), i1.value, i2.value] == r[2], d
        assert [lib.viai_conv2d_packed_floats(C.byref(c)), lib.viai_conv2d_wgrad_ws_bytes(C.byref(c)), lib.viai_conv2d_fwd_f16_ok(C.byref(c)),
                lib.viai_conv2d_dgrad_f16_ok(C.byref(c)), lib.viai_conv2d_wgrad_f16_ok(C.byref(c)), lib.viai_conv2d_p16_ok(C.byref(c))] == r[3:9], d
        for dg in (0, 1, 2):
            j = PackJob()
            rc = lib.viai_conv2d_pack_job(C.byref(c), dg, None, None, C.byref(j))
            assert [rc] + ([j.frag, j.n_out, j.k_in, j.s_no, j.s_ki, j.nblk] if rc == 0 else [0] * 6) == r[9 + dg], (d, dg)


def test_route_names_the_recorded_kernel(lib):
    from viai_amd._lib import Conv2dDesc
    tool = _tool()
    buf = C.create_string_buffer(64)
    checked = 0
    for r in ROWS:
        d = r[0]
        if len(r) < 21:
            continue
        c = Conv2dDesc(*_desc17(d))
        for i, (rc, n, fam) in enumerate(r[12:21]):
            p, f = tool.pass_form(i, d)
            rn = lib.viai_conv2d_route(C.byref(c), p, f, buf, 64)
            got = (rn, buf.value.decode())
            if _cin1_without_kernel(d):
                assert got == (0, ""), (d, tool.LAUNCHES[i], got)
            elif rc == NO_DEVICE and p == 1 and d[8] * d[9] > 1 and not fam.startswith("dgrad_s2") and fam != "direct":
                # class by class: the recorded call stopped at its first launch, so only the arithmetic of the family is comparable; the
                # count is one launch per live class
                assert rn == _live_classes(d) and got[1].rsplit("_", 1)[1] == fam.rsplit("_", 1)[1], (d, tool.LAUNCHES[i], got, fam)
            elif rc == NO_DEVICE:
                assert got == (n, fam), (d, tool.LAUNCHES[i], got, (n, fam))
            elif n == 0 and not (p == 1 and tool.tapless_class(d)):
                assert got == (0, ""), (d, tool.LAUNCHES[i], got)      # refused before any kernel was chosen
            elif fam == "direct":
                assert (rc, n) == (1, 1) and got == (1, "direct"), (d, tool.LAUNCHES[i], got)     # tagged, then refused by the streaming kernel's own checks: the route answers like the tag
            else:
                assert p == 1 and rc == 1 and n == 0 and tool.tapless_class(d), (d, tool.LAUNCHES[i], rc, n, fam)     # failed at the zero-fill: nothing recorded to compare
                continue
            checked += 1
    assert checked > 1200
