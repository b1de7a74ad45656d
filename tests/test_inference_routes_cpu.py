"""The inference shape table, held to the kernels it was chosen for.  No GPU: viai_conv2d_route, viai_conv2d_stat_tiles and
viai_pair_cout1_ok are host code.

AudioModel.test() runs the generator (MelEncoder + MelDecoder) in eval mode, every conv through viai_conv2d_fwd_amax on fp32 operands; the fp32
form (viai_conv2d_fwd) must route the same way.  tests/inference_common.py derives the layers of a (B, F, T) clip from the modules; here the table
as a whole must reach every condition of inference_common.CONDITIONS plus both answers of the pair query, and each shape must still reach
what REACHES records for it -- so a route change that moves a shape off its kernel, or a shape swapped for one where every tile is full
(T = 256 reaches none of the ragged conditions), fails here and not silently on the GPU.

halo_wide32_f16x2 with OH % 8 != 0: legal shapes do give it.  With 80 mel bands the 32-channel maps are 20, 40 and 80 rows high and only
G.cb4 (20 rows) is off the 8-row tile; the route takes the wide halo kernel from M = N * 20 * ceil(T / 2) of about 18 000 pixels, so 8 streams
of T >= 225 frames (4 of T >= 449) reach it, G.cb4_0 with its virtual concat included.  (8, 80, 225) is in the table for that.  Other band
counts reach it on G.conv6_1 (8 x 68 x 34).
"""
import pytest

import inference_common as IC

PAIR, NO_PAIR = "Cout = 1 pair fused", "Cout = 1 pair as two layers"
SK_RAG, SK_SMALL = "igemm_sk32x32_f16x2 at M % 32 != 0", "igemm_sk32x32_f16x2 at M < 32"
IG_RAG, IG_CAT = "igemm128x32_f16x2 at M % 128 != 0", "igemm128x32_f16x2 with a virtual concat at ragged M"
W_RIGHT, W_BELOW = "halo_wide32_f16x2 with (8, 16) tiles clipped on the right", "halo_wide32_f16x2 with (8, 16) tiles clipped below"
C32, CIN1_ODD = "halo_c32_f16x2", "Cin = 1 direct at odd width and stride 2"

# what each shape reaches, as the library answered when the table was made
REACHES = {
    (4, 80, 100): {SK_RAG, IG_RAG, IG_CAT, W_RIGHT, NO_PAIR},
    (1, 80, 345): {SK_RAG, IG_RAG, IG_CAT, W_RIGHT, CIN1_ODD, NO_PAIR},
    (8, 80, 208): {SK_RAG, W_RIGHT, C32, PAIR},
    (2, 80, 37): {SK_RAG, SK_SMALL, IG_RAG, IG_CAT, CIN1_ODD, NO_PAIR},
    (1, 80, 61): {SK_RAG, SK_SMALL, IG_RAG, IG_CAT, CIN1_ODD, NO_PAIR},
    (1, 80, 7): {SK_RAG, SK_SMALL, IG_RAG, IG_CAT, CIN1_ODD, NO_PAIR},
    (1, 80, 1): {SK_RAG, SK_SMALL, IG_RAG, IG_CAT, CIN1_ODD, NO_PAIR},
    (2, 68, 32): {SK_RAG, SK_SMALL, IG_RAG, IG_CAT, PAIR},
    (8, 80, 225): {SK_RAG, W_RIGHT, W_BELOW, CIN1_ODD, NO_PAIR},
}
RAGGED = {SK_RAG, SK_SMALL, IG_RAG, IG_CAT, W_RIGHT, W_BELOW}


@pytest.fixture(scope="module")
def lib():
    from viai_amd import _lib
    return _lib.load()


def reached(lib, shape):
    layers = IC.generator_layers(*shape)
    got = {PAIR if IC.pair_ok(lib, layers) else NO_PAIR}
    for l in layers:
        fam, n = IC.route(lib, l.desc, 1)
        assert n == 1 and fam, (shape, l)
        assert IC.route(lib, l.desc, 0) == (fam, n), (shape, l)           # the fp32 form routes like the abs-max form
        tiles = IC.stat_tiles(lib, l.desc)
        got.update(name for name, cond in IC.CONDITIONS.items() if cond(fam, l.desc, l.M, l.OH, l.OW, tiles))
    return got


def test_the_layer_walk_matches_the_modules():
    """22 convs; shapes chain; the maps of the timed step come out as tests/test_fullsize_gpu.py lists them"""
    L = IC.generator_layers(16, 256, 256)
    assert [l.name for l in L][:7] == ["E.conv1", "E.conv2", "E.conv3", "E.conv4", "E.conv5", "G.deconv1_1", "G.deconv1_2"] and len(L) == 22
    by = {l.name: l for l in L}
    assert by["E.conv2"].desc[:13] == (16, 128, 128, 32, 0, 64, 3, 3, 2, 1, 1, 1, 0)
    assert by["G.deconv1_1"].desc[:13] == (16, 2, 16, 256, 0, 256, 3, 3, 1, 1, 0, 1, 1) and (by["G.deconv1_1"].OH, by["G.deconv1_1"].OW) == (4, 16)
    assert by["G.cb4_0"].desc[:13] == (16, 64, 128, 64, 64, 32, 3, 3, 1, 1, 1, 1, 1)
    assert by["G.conv6_2"].desc[:13] == (16, 256, 256, 32, 0, 1, 3, 3, 1, 1, 1, 1, 1)
    one = {l.name: l for l in IC.generator_layers(1, 80, 1)}
    assert one["G.deconv1_1"].desc[:3] == (1, 1, 1) and one["G.deconv1_1"].M == 3 and one["E.conv5"].M == 3


def test_the_table_reaches_every_condition(lib):
    assert len(IC.INFERENCE_SHAPES) == len(set(IC.INFERENCE_SHAPES)) == len(REACHES)
    total = set()
    for shape in IC.INFERENCE_SHAPES:
        assert shape in REACHES, "%s is not a shape this table was chosen with: say what it reaches in REACHES" % (shape,)
        got = reached(lib, shape)
        assert got == REACHES[shape], "%s: no longer %s, newly %s" % (shape, sorted(REACHES[shape] - got), sorted(got - REACHES[shape]))
        assert got & RAGGED, "%s: every tile of every layer is full" % (shape,)
        total |= got
    want = set(IC.CONDITIONS) | {PAIR, NO_PAIR}
    assert total == want, "not reached by any shape: %s" % sorted(want - total)


def test_a_shape_of_full_tiles_would_be_caught(lib):
    """the timed step's shape, and a clip of T = 256: no ragged condition"""
    for shape in ((16, 256, 256), (4, 80, 256)):
        assert not (reached(lib, shape) & RAGGED), shape
