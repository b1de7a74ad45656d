"""The contrastive loss (csrc/contrastive.hip) and the batch / retrieval passes (csrc/pipeline.hip) called directly at the C ABI and compared with
an fp64 restatement on the CPU (tests/passes_common.py: how the bounds are made; tests/contrastive_common.py: the truths, the planted ties and the
condition under which a discrete decision may be compared exactly; tests/test_contrastive_inputs_cpu.py checks that condition without a GPU).

Branch table -- one row per launch, the parametrisation that reaches each branch:

  launch                    branch                                                    reached by
  l2c_scores_kernel         n % 4 = 1, 2, 1, 2, 0, 1, 0: waves with b >= n return     test_l2c n = 1, 2, 5, 6, 64, 257, 300 (n = 1: three of four waves idle;
                                                                                      n % 4 = 3 has no n of the issue's list: test_l2c_scores_n7, n = 7)
                            d < 64 / = 64 / % 64 != 0 / > 256                         test_l2c d = 1, 63 / 64 / 65, 300 / 300 (each n with two or three d)
  l2c_loss_kernel           n < 256: idle threads; n > 256: a thread sums two rows    test_l2c n <= 64; n = 257, 300
                            max_violation 0 / 1                                       test_l2c, both at every shape and margin
                            no active hinge anywhere (loss = diagonal term)           test_l2c margin "zero" (0, the module's default)
                            a row with no active hinge                                test_l2c margin "row" (below the smallest distance of the far row)
                            part of the hinges active / every hinge active            test_l2c margin "mid" / "all"
  l2c_argmax_kernel         one block / two blocks                                    test_l2c n <= 64 / n = 257, 300: argmax_ws read back, compared exactly
                            planted tie: the lower index wins                         test_l2c n >= 5, "mid" and "all": arg[a0] = p, not q
                            row with no violation: the first b != a                   test_l2c "zero" (every row; row 0 gives 1), "row" (the far row)
                            n = 1: arg = -1                                           test_l2c n = 1
                            not launched without max_violation                        test_l2c: argmax_ws keeps its sentinel
  l2c_bwd_kernel which 0, 1 d < 256: idle threads / d = 300: two columns per thread   test_l2c d <= 256 / d = 300
                            zero distance on the diagonal (z, z) and off it (x, y)    test_l2c n >= 5: finite, and exactly 0 where nothing else contributes
                            gscale NULL / device scalar                               test_l2c alternates; test_l2c_bwd_outputs_and_gscale: both, every output set
                            df1 only / df2 only / both                                test_l2c_bwd_outputs_and_gscale: the buffer not asked for keeps its sentinel
                            inactive hinges (c <= 0), non-arg-max columns             test_l2c margins "zero", "row", "mid"; max_violation 1
  viai_l2c_fwd / _bwd       n <= 0, d <= 0 refused before any launch                  test_l2c_refusals: sentinels intact, no error left after a synchronize
  frames_prep_kernel        C = 1, 2, 3, 4: channels C.. exactly +0                   test_frames_prep C, bitwise (a -0 would differ)
                            flip 0 / 1                                                test_frames_prep flip
                            crop at 0 and at S - size on both axes                    test_frames_prep crops (0,0) (4,4) (0,4) (4,0), S = 9, size = 5
                            size == S                                                 test_frames_prep S = size = 7
                            8192-block cap reached, grid-stride wraps                 test_frames_prep_wrapped: 42 frames of 224 x 224 out of 230 x 230
                            refusals                                                  test_frames_prep_refusals: C = 0, 5; size 0; crop < 0; crop + size > S
  slice_clips_kernel        start 0 / straddles the end / wholly past the end         test_slice_clips starts 0, 12, 13 and 40 (T_total = 55, L = 8)
                            last valid frame exactly at T_total - 1                   test_slice_clips start 11 (frames 47..54)
                            samples < T_total * hop                                   test_slice_clips: 10 samples short, the audio of start 11 pads, its mel not
                            both halves of the index space in one wrapped grid        test_slice_clips_wrapped B = 13, L = 512, D = 80, hop = 256
                            refusals                                                  test_slice_clips_refusals B, D, L, hop = 0
  ema_kernel                one block / wrapped grid                                  test_ema n = 1, 255, 8192 * 256 + 777
                            decay 0.9999, 0.9 / 0.0 / 1.0                             test_ema: measured / equals x within the bound / unchanged bit for bit
                            five successive updates in place                          test_ema, every step against the fp64 chain
  mel_denorm_amp_kernel     clamp edges: S < 0, > 1, = 0, = 1                         test_mel_denorm_amp (planted at the head and the tail of the tensor)
                            NaN: fmaxf(NaN, 0) = 0, so NaN -> the floor amplitude     test_mel_denorm_amp: bit for bit the output of S = 0
                                                                                      (np.clip would hand the NaN on; the kernel does not, and this pins it)
                            min_level_db -100 / -80                                   test_mel_denorm_amp
                            wrapped grid                                              test_mel_denorm_amp n = 8192 * 256 + 777
  l2_ranks_kernel           n_clips < 256 (threads that see no clip carry the         test_l2_ranks n_clips = 1, 5, 255
                            sentinel into the reduction) / = 256 / two, three strides test_l2_ranks n_clips = 256 / 257, 700
                            n_captions == n_clips / < n_clips                         test_l2_ranks, both at every n_clips >= 5
                            dim 1 / 64 / 8192 (the limit; 32 KiB of dynamic LDS)      test_l2_ranks dim (8192 at n_clips = 5)
                            ties decided by index: j < i counts, j > i does not;      test_l2_ranks planted copies below and above the matching clip, the
                            the lower index is top-1                                  duplicated nearest clip, and every natural tie of the grid family
                            dist NULL / set                                           test_l2_ranks, both at every case
                            refusals                                                  test_l2_ranks_refusals n_captions 0, > n_clips; dim 0, 8193

Why each named case alone notices its branch broken (no GPU run of a broken kernel was made):
  * drop `b >= n` in the scores kernel: the surplus waves of the last block row store past scores[a][n - 1], i.e. into scores[a + 1][0..] (caught by
    every n % 4 != 0, the element is overwritten with a distance to a row of f2 that does not exist) and past the end at a = n - 1;
  * `c > best` -> `c >= best` in the arg-max: arg[a0] becomes q (the LAST maximum) at "mid" / "all", and the zero-violation rows give n - 1 or n - 2;
  * remove `sc <= 0` in l2c_w: w = -margin / (n * 0) = -inf at (x, y), inf * 0 = NaN in df1[x] and df2[y] (the differences are exactly 0);
  * drop `j < i` in l2_ranks: rank[i0] loses the planted copy below it; `j <= i` or an unconditional tie count adds the copy above;
  * cap a grid without the stride loop: everything past element 8192 * 256 keeps its NaN sentinel in the four wrapped cases;
  * an idle thread that contributes (loss n < 256, ranks n_clips < 256, a sentinel of 0 instead of 3.4e38 / INT_MAX): top-1 becomes INT_MAX or a
    wrong index at n_clips = 1, 5, 255.

Worst errors measured on the MI355X: MEASURED below.  No kernel defect was found.  One case missed its bound on the first run, and the fault
was the test's: dist at dim = 8192 erred by 7.8e-5 (9e-7 relative) against a bound of 2.0e-5 made from torch's pairwise sum(), which is a more
accurate formula than the one the kernel states (one accumulator, coordinate after coordinate: about sqrt(8192) roundings).  The fp32 restatement
of the squared distance now adds in that order too (contrastive_common.ret_d2), THE CONDITION of the rank decisions is measured with it, and the
same case stands at 0.25 of its bound.
"""
import math

import numpy as np
import pytest
import torch

import contrastive_common as C
from oracle import pipeline_oracle as P
from passes_common import EPS32, INVALID, assert_bitwise, bound_abs, check_abs, check_rel, dev, host, lib, ok, ptr, st, uniform

pytestmark = pytest.mark.gpu

# worst error measured on the MI355X per pass family (the bounds themselves are made per case from the fp32 restatement: passes_common)
MEASURED = {       # worst (error / bound) over the cases, and that case's error
    "l2c scores": "0.30 of the bound: 1.8e-6 abs on distances of 15 at n = 257, d = 65",
    "l2c loss": "0.59 of the bound: 2.9e-6 abs at n = 1, d = 64, margin 'all', max_violation (one squared score; the kernel sums in fp64)",
    "l2c df1 / df2": "0.45 of the bound: 1.4e-6 abs at df1, n = 6, d = 64, margin 'all', every hinge summed",
    "ema": "0.29 of the bound: 7.7e-8 abs at n = 255, decay 0.9, fourth update; decay 0 and 1 are exact",
    "mel_denorm_amp": "0.25 of the bound: 5.9e-7 relative at n = 300, min_level_db -80: the device exp10f needs no wider bound than the restatement gives",
    "l2_ranks dist": "0.25 of the bound: 7.8e-5 abs on distances of 83 at 5 clips, dim 8192 (2.2e-6 abs at 700 clips, dim 64)",
}

CAP = 8192 * 256                # elements one pass of a capped element-wise grid covers (viai_ew_blocks)
NAN = float("nan")
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    for fam in sorted(WORST):
        print("WORST %-14s %.3f of the bound: %.3e at %s" % ((fam,) + WORST[fam]))


def _abs(fam, got, ref64, f32, what):
    err = check_abs(got, ref64, f32, what)
    b = bound_abs(ref64, f32)
    ratio = 0.0 if err == 0.0 else err / b
    if ratio >= WORST.get(fam, (-1.0,))[0]:
        WORST[fam] = (ratio, err, what)


def _rel(fam, got, ref64, f32, what):
    worst = check_rel(got, ref64, f32, what)
    rel = max(4.0 * float(((f32.double() - ref64).abs() / ref64.abs().clamp_min(1e-300)).max()), 2.0 * EPS32)
    if worst / rel >= WORST.get(fam, (-1.0,))[0]:
        WORST[fam] = (worst / rel, worst, what)


def _no_error_left():
    torch.cuda.synchronize()
    assert float(torch.ones(1, device="cuda").sum()) == 1.0


# ---------------------------------------------------------------------------------------------------------------- contrastive loss

def _l2c_fwd(f1, f2, margin, mv):
    L = lib()
    n, d = f1.shape
    f1d, f2d = dev(f1), dev(f2)
    scores = torch.full((n, n), NAN, device="cuda")
    loss = torch.full((1,), NAN, device="cuda")
    ok(L.viai_l2c_fwd(f1d.data_ptr(), f2d.data_ptr(), n, d, margin, mv, scores.data_ptr(), loss.data_ptr(), st()), "viai_l2c_fwd")
    return f1d, f2d, scores, loss


def _l2c_bwd(f1d, f2d, scores, margin, mv, gs, want1=True, want2=True):
    L = lib()
    n, d = f1d.shape
    arg = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    df1 = torch.full((n, d), NAN, device="cuda")
    df2 = torch.full((n, d), NAN, device="cuda")
    gsd = None if gs is None else torch.tensor([gs], device="cuda")
    ok(L.viai_l2c_bwd(f1d.data_ptr(), f2d.data_ptr(), scores.data_ptr(), n, d, margin, mv, ptr(gsd), arg.data_ptr(),
                      df1.data_ptr() if want1 else 0, df2.data_ptr() if want2 else 0, st()), "viai_l2c_bwd")
    return host(arg), host(df1), host(df2)


@pytest.mark.parametrize("n,d", C.L2C_SHAPES)
def test_l2c(n, d):
    f1, f2, s64, s32, _ = C.l2c_scores(n, d)
    pl = C.l2c_plan(n)
    for ki, kind in enumerate(C.MARGIN_KINDS):
        margin = C.l2c_margin(s64, kind)
        for mv in (0, 1):
            gs = (None, 3.0)[(ki + mv) % 2]
            g = 1.0 if gs is None else gs
            tag = "n=%d d=%d %s mv=%d" % (n, d, kind, mv)
            r64 = C.l2c_ref64(f1, f2, s64, margin, mv, g)
            r32 = C.l2c_ref32(f1, f2, s32, margin, mv, g)
            f1d, f2d, scores, loss = _l2c_fwd(f1, f2, margin, mv)
            if ki == 0 and mv == 0:
                _abs("l2c scores", scores, s64, s32, "l2c scores n=%d d=%d" % (n, d))
                if pl is not None:
                    sh = host(scores)
                    assert float(sh[pl["z"], pl["z"]]) == 0.0 and float(sh[pl["x"], pl["y"]]) == 0.0
                    assert_bitwise(sh[:, pl["p"]], sh[:, pl["q"]], "scores of the duplicated rows")
            _abs("l2c loss", loss, r64["loss"], r32["loss"], "l2c loss " + tag)
            arg, df1, df2 = _l2c_bwd(f1d, f2d, scores, margin, mv, gs)
            if mv:
                assert np.array_equal(arg.numpy(), r64["arg"]), (tag, arg.numpy(), r64["arg"])
            else:
                assert bool((arg == -7).all())                               # no arg-max launch without max_violation
            assert bool(torch.isfinite(df1).all()) and bool(torch.isfinite(df2).all()), tag
            _abs("l2c df", df1, r64["df1"], r32["df1"], "l2c df1 " + tag)
            _abs("l2c df", df2, r64["df2"], r32["df2"], "l2c df2 " + tag)
            if pl is not None and kind == "zero":
                # only the diagonal contributes, and at (z, z) the distance is 0: nothing at all
                assert bool((df1[pl["z"]] == 0).all()) and bool((df2[pl["z"]] == 0).all())
            if pl is not None and mv and kind in ("mid", "all"):
                assert arg[pl["a0"]] == pl["p"] and arg[pl["x"]] == pl["y"]


def test_l2c_scores_n7():
    """n % 4 = 3 (one idle wave in the last block row); no n of the other cases leaves that remainder"""
    n, d = 7, 65
    f1, f2 = uniform("l2c.n7.f1", (n, d)), uniform("l2c.n7.f2", (n, d))
    _, _, scores, _ = _l2c_fwd(f1, f2, 0.0, 0)
    _abs("l2c scores", scores, C.scores_of(f1, f2, torch.float64), C.scores_of(f1, f2, torch.float32), "l2c scores n=7 d=65")


@pytest.mark.parametrize("n,d", [(5, 65), (6, 300), (257, 64)])
def test_l2c_bwd_outputs_and_gscale(n, d):
    f1, f2, s64, s32, _ = C.l2c_scores(n, d)
    margin = C.l2c_margin(s64, "mid")
    for mv in (0, 1):
        f1d, f2d, scores, _ = _l2c_fwd(f1, f2, margin, mv)
        for gs in (None, 3.0):
            g = 1.0 if gs is None else gs
            r64 = C.l2c_ref64(f1, f2, s64, margin, mv, g)
            r32 = C.l2c_ref32(f1, f2, s32, margin, mv, g)
            for want1, want2 in ((True, False), (False, True), (True, True)):
                tag = "n=%d d=%d mv=%d gs=%s out=%d%d" % (n, d, mv, gs, want1, want2)
                arg, df1, df2 = _l2c_bwd(f1d, f2d, scores, margin, mv, gs, want1, want2)
                if want1:
                    _abs("l2c df", df1, r64["df1"], r32["df1"], "l2c df1 " + tag)
                else:
                    assert bool(torch.isnan(df1).all())
                if want2:
                    _abs("l2c df", df2, r64["df2"], r32["df2"], "l2c df2 " + tag)
                else:
                    assert bool(torch.isnan(df2).all())


def test_l2c_refusals():
    L = lib()
    f = torch.ones(4, 4, device="cuda")
    scores = torch.full((4, 4), -5.0, device="cuda")
    loss = torch.full((1,), -5.0, device="cuda")
    arg = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    df1, df2 = torch.full((4, 4), -5.0, device="cuda"), torch.full((4, 4), -5.0, device="cuda")
    for n, d in ((0, 4), (-1, 4), (4, 0), (4, -3)):
        assert L.viai_l2c_fwd(f.data_ptr(), f.data_ptr(), n, d, 1.0, 1, scores.data_ptr(), loss.data_ptr(), st()) == INVALID
        assert L.viai_l2c_bwd(f.data_ptr(), f.data_ptr(), scores.data_ptr(), n, d, 1.0, 1, 0, arg.data_ptr(), df1.data_ptr(), df2.data_ptr(), st()) == INVALID
    _no_error_left()
    assert bool((scores == -5).all()) and float(loss) == -5.0 and bool((arg == -7).all()) and bool((df1 == -5).all()) and bool((df2 == -5).all())


# ---------------------------------------------------------------------------------------------------------------- frames_prep

def _bytes(tag, shape):
    return uniform(tag, shape, 0.0, 256.0).floor().clamp(0, 255).to(torch.uint8)


def _frames_ref(fr, size, cx, cy, flip):
    """flip left to right, rows [cx, +size), columns [cy, +size), (px - 127) / 128 (exact in fp32), channels C.. = +0"""
    n, S, _, Cc = fr.shape
    f = fr.to(torch.float32)
    if flip:
        f = f.flip(2)
    out = torch.zeros(n, size, size, 4)
    out[..., :Cc] = (f[:, cx:cx + size, cy:cy + size, :] - 127.0) / 128.0
    return out


def _frames_run(fr, size, cx, cy, flip):
    n, S, _, Cc = fr.shape
    out = torch.full((n, size, size, 4), NAN, device="cuda")
    frd = fr.cuda()
    ok(lib().viai_frames_prep(frd.data_ptr(), out.data_ptr(), n, S, Cc, size, cx, cy, flip, st()), "viai_frames_prep")
    return out


@pytest.mark.parametrize("Cc", [1, 2, 3, 4])
@pytest.mark.parametrize("flip", [0, 1])
def test_frames_prep(Cc, flip):
    for S, size, crops in ((9, 5, ((0, 0), (4, 4), (0, 4), (4, 0), (1, 2))), (7, 7, ((0, 0),))):
        fr = _bytes("fp.%d.%d" % (S, Cc), (3, S, S, Cc))
        for cx, cy in crops:
            want = _frames_ref(fr, size, cx, cy, flip)
            assert_bitwise(_frames_run(fr, size, cx, cy, flip), want, "frames_prep C=%d flip=%d S=%d crop=(%d,%d)" % (Cc, flip, S, cx, cy))
            if Cc <= 3 and flip == 1 and (cx, cy) == (1, 2):                 # the restatement against the oracle's own
                assert np.array_equal(want[..., :Cc].permute(0, 3, 1, 2).numpy(), P.frames_prep(fr.numpy(), size, cx, cy, True))


def test_frames_prep_wrapped():
    n, S, size = 42, 230, 224
    assert n * size * size == 2107392 > CAP
    fr = _bytes("fp.big", (n, S, S, 3))
    assert_bitwise(_frames_run(fr, size, S - size, S - size, 1), _frames_ref(fr, size, S - size, S - size, 1), "frames_prep 42 x 224 x 224")


def test_frames_prep_refusals():
    L = lib()
    fr = torch.zeros(2, 9, 9, 4, dtype=torch.uint8, device="cuda")
    out = torch.full((2, 9, 9, 4), -5.0, device="cuda")
    for Cc, size, cx, cy in ((0, 5, 0, 0), (5, 5, 0, 0), (3, 0, 0, 0), (3, -1, 0, 0), (3, 5, -1, 0), (3, 5, 0, -1), (3, 5, 5, 0), (3, 5, 0, 5), (3, 10, 0, 0)):
        assert L.viai_frames_prep(fr.data_ptr(), out.data_ptr(), 2, 9, Cc, size, cx, cy, 0, st()) == INVALID, (Cc, size, cx, cy)
    _no_error_left()
    assert bool((out == -5).all())


# ---------------------------------------------------------------------------------------------------------------- slice_clips

def _slice_ref(c, x, starts, L, hop):
    """clip b: mel frames [3 + 4 start, +L) transposed to (D, L), samples [(3 + 4 start) hop, +L hop); zeros past either end"""
    D = c.shape[1]
    co, xo = torch.zeros(len(starts), D, L), torch.zeros(len(starts), L * hop)
    for b, s in enumerate(starts):
        m0 = 3 + 4 * s
        seg, xs = c[m0:m0 + L], x[m0 * hop:(m0 + L) * hop]
        co[b, :, :seg.shape[0]] = seg.t()
        xo[b, :xs.shape[0]] = xs
    return co, xo


def _slice_run(c, x, starts, L, hop):
    T_total, D = c.shape
    B = len(starts)
    cd, xd = dev(c), dev(x)
    sd = torch.tensor(starts, dtype=torch.int32, device="cuda")
    co, xo = torch.full((B, D, L), NAN, device="cuda"), torch.full((B, L * hop), NAN, device="cuda")
    ok(lib().viai_slice_clips(cd.data_ptr(), xd.data_ptr(), sd.data_ptr(), co.data_ptr(), xo.data_ptr(), B, D, L, hop, T_total, x.numel(), st()),
       "viai_slice_clips")
    return co, xo


def test_slice_clips():
    T_total, D, L, hop = 55, 5, 8, 7
    c = uniform("sc.c", (T_total, D))
    x = uniform("sc.x", (T_total * hop - 10,))               # the audio ends 10 samples before the mel does
    starts = [0, 11, 12, 13, 40, 11]
    assert 3 + 4 * 11 + L - 1 == T_total - 1 and 3 + 4 * 12 < T_total < 3 + 4 * 12 + L and 3 + 4 * 13 == T_total
    wc, wx = _slice_ref(c, x, starts, L, hop)
    assert float(wc[1].abs().min()) > 0 and bool((wx[1, -10:] == 0).all()) and float(wx[1, :-10].abs().min()) > 0      # the mel whole, the audio padded
    assert bool((wc[3] == 0).all()) and bool((wx[3] == 0).all()) and bool((wc[4] == 0).all())                        # wholly past the end
    assert bool((wc[2, :, :4] != 0).all()) and bool((wc[2, :, 4:] == 0).all())                                       # straddles it
    cb, xb = P.slice_clips(c.numpy(), x.numpy(), starts, L // 4, hop)
    assert np.array_equal(cb, wc.numpy()) and np.array_equal(xb[:, 0], wx.numpy())                                   # the restatement against the oracle's own
    gc, gx = _slice_run(c, x, starts, L, hop)
    assert_bitwise(gc, wc, "slice_clips mel")
    assert_bitwise(gx, wx, "slice_clips audio")


def test_slice_clips_wrapped():
    B, L, D, hop, T_total = 13, 512, 80, 256, 1199
    assert B * D * L < CAP < B * L * (D + hop)                # the boundary between the two halves lies inside the first pass, the wrap in the audio
    c = uniform("sc.big.c", (T_total, D))
    x = uniform("sc.big.x", (T_total * hop - 100,))
    starts = [0, 20, 41, 63, 84, 105, 126, 147, 171, 172, 190, 299, 300]          # 171: last frame at T_total - 1; from 172 on: straddling, then past
    assert 3 + 4 * 171 + L == T_total
    wc, wx = _slice_ref(c, x, starts, L, hop)
    gc, gx = _slice_run(c, x, starts, L, hop)
    assert_bitwise(gc, wc, "slice_clips mel, wrapped")
    assert_bitwise(gx, wx, "slice_clips audio, wrapped")


def test_slice_clips_refusals():
    L = lib()
    z = torch.full((64,), -5.0, device="cuda")
    s = torch.zeros(4, dtype=torch.int32, device="cuda")
    for B, D, Ln, hop in ((0, 2, 2, 2), (2, 0, 2, 2), (2, 2, 0, 2), (2, 2, 2, 0), (-1, 2, 2, 2)):
        assert L.viai_slice_clips(z.data_ptr(), z.data_ptr(), s.data_ptr(), z.data_ptr(), z.data_ptr(), B, D, Ln, hop, 16, 32, st()) == INVALID
    _no_error_left()
    assert bool((z == -5).all())


# ---------------------------------------------------------------------------------------------------------------- EMA

@pytest.mark.parametrize("n", [1, 255, CAP + 777])
@pytest.mark.parametrize("decay", [0.9999, 0.9, 0.0, 1.0])
def test_ema(n, decay):
    """shadow -= (1 - decay) * (shadow - x) with (1 - decay) rounded once to fp32 (include/viai_hip.h, csrc/pipeline.hip); five updates in place"""
    L = lib()
    omd = float(np.float32(1.0 - decay))
    s0 = uniform("ema.s", (n,))
    s64, s32 = s0.double(), s0.clone()
    sd = dev(s0)
    for t in range(5):
        x = uniform("ema.x%d" % (t % 2), (n,)) * (1.0 + 0.5 * t)
        xd = dev(x)
        ok(L.viai_ema_update(sd.data_ptr(), xd.data_ptr(), n, decay, st()), "viai_ema_update")
        s64 = s64 - omd * (s64 - x.double())
        s32 = s32 - torch.tensor(omd, dtype=torch.float32) * (s32 - x)
        if decay == 1.0:
            assert_bitwise(sd, s0, "ema decay=1 step %d" % (t + 1))
        else:
            _abs("ema", sd, s64, s32, "ema n=%d decay=%g step %d" % (n, decay, t + 1))
        if decay == 0.0:
            assert float((s64 - x.double()).abs().max()) <= 2.0 ** -50 * float(x.abs().max())       # the truth IS x there


# ---------------------------------------------------------------------------------------------------------------- inverse mel

def _mel_v(S, mld, dtype):
    s = torch.where(torch.isnan(S), torch.zeros_like(S), S).to(dtype).clamp(0.0, 1.0)          # fmaxf(NaN, 0) = 0: the kernel's rule for NaN
    return s * torch.tensor(-mld, dtype=dtype) + torch.tensor(mld, dtype=dtype)


def _mel64(S, mld):
    return torch.pow(torch.tensor(10.0, dtype=torch.float64), _mel_v(S, mld, torch.float64) / 20.0)


def _mel32(S, mld):
    return torch.pow(torch.tensor(10.0, dtype=torch.float32), _mel_v(S, mld, torch.float32) * torch.tensor(0.05, dtype=torch.float32))


@pytest.mark.parametrize("n", [300, CAP + 777])
@pytest.mark.parametrize("mld", [-100.0, -80.0])
def test_mel_denorm_amp(n, mld):
    L = lib()
    S = uniform("mel.S", (n,), -0.2, 1.2).clone()
    edges = torch.tensor([0.0, 1.0, -0.0, -3.0, 7.0, 2.0 ** -30, 1.0 - 2.0 ** -24, 1.0 + 2.0 ** -23, NAN, -1e-30, float("inf"), float("-inf")])
    S[:edges.numel()] = edges
    S[-edges.numel():] = edges
    out = torch.full((n,), NAN, device="cuda")
    Sd = dev(S)
    ok(L.viai_mel_denorm_amp(Sd.data_ptr(), out.data_ptr(), n, mld, st()), "viai_mel_denorm_amp")
    got = host(out)
    assert bool(torch.isfinite(got).all())
    ref = _mel64(S, mld)
    assert abs(float(ref[0]) / 10.0 ** (mld / 20.0) - 1.0) <= 1e-15 and float(ref[1]) == 1.0 and float(ref.max()) == 1.0 and float(ref.min()) == float(ref[0])
    _rel("mel", got, ref, _mel32(S, mld), "mel_denorm_amp n=%d min_level_db=%g" % (n, mld))
    # clamp edges land exactly where S = 0 and S = 1 do; NaN goes to the floor, as S = 0
    for base in (0, n - edges.numel()):
        g = got[base:base + edges.numel()].view(torch.int32).tolist()
        assert g[2] == g[0] and g[3] == g[0] and g[9] == g[0] and g[11] == g[0], "below 0"
        assert g[4] == g[1] and g[7] == g[1] and g[10] == g[1], "above 1"
        assert g[8] == g[0], "NaN -> floor amplitude"


# ---------------------------------------------------------------------------------------------------------------- retrieval

def _ranks_run(clips, caps, with_dist):
    n_clips, dim = clips.shape
    n_cap = caps.shape[0]
    cd, qd = dev(clips), dev(caps)
    ranks = torch.full((n_cap,), -7, dtype=torch.int32, device="cuda")
    top1 = torch.full((n_cap,), -7, dtype=torch.int32, device="cuda")
    dist = torch.full((n_cap, n_clips), NAN, device="cuda") if with_dist else None
    ok(lib().viai_l2_ranks(cd.data_ptr(), qd.data_ptr(), n_clips, n_cap, dim, ranks.data_ptr(), top1.data_ptr(), ptr(dist), st()), "viai_l2_ranks")
    return host(ranks).numpy(), host(top1).numpy(), dist


@pytest.mark.parametrize("case", C.RET_CASES, ids=lambda c: "%d-%d-%d-%s" % c)
def test_l2_ranks(case):
    n_clips, n_cap, dim, family = case
    clips, caps, d64, d32, _ = C.ret_truth(*case)
    _, ranks, top1 = P.l2_retrieval(clips.numpy(), caps.numpy())             # a stable sort of the fp64 distances
    for with_dist in (False, True):
        r, t, dist = _ranks_run(clips, caps, with_dist)
        assert np.array_equal(r, ranks), (case, with_dist, np.nonzero(r != ranks)[0][:8], r[:8], ranks[:8])
        assert np.array_equal(t, top1), (case, with_dist, np.nonzero(t != top1)[0][:8], t[:8], top1[:8])
        if with_dist:
            _abs("ranks dist", dist, d64.sqrt(), d32.sqrt(), "l2_ranks dist %d-%d-%d-%s" % case)
    pl = C.ret_plan(n_clips, n_cap)
    if pl is not None:
        assert top1[pl["i1"]] <= pl["k1"] and ranks[pl["i0"]] >= 1


def test_l2_ranks_refusals():
    L = lib()
    z = torch.full((16, 4), -5.0, device="cuda")
    r = torch.full((16,), -7, dtype=torch.int32, device="cuda")
    t = torch.full((16,), -7, dtype=torch.int32, device="cuda")
    for n_clips, n_cap, dim in ((4, 0, 4), (4, -1, 4), (4, 5, 4), (4, 4, 0), (4, 4, -1), (4, 4, 8193)):
        assert L.viai_l2_ranks(z.data_ptr(), z.data_ptr(), n_clips, n_cap, dim, r.data_ptr(), t.data_ptr(), z.data_ptr(), st()) == INVALID
    _no_error_left()
    assert bool((z == -5).all()) and bool((r == -7).all()) and bool((t == -7).all())
