"""The host-side decisions of viai_amd/ops.py, pinned without a GPU.  Nothing is launched.

  * `ops._dy_form` -- in which form a fused layer's dy leaves its BatchNorm backward, and whether the pass reduces max |dy| -- is compared over its
    WHOLE input space with the expressions it replaced: the four predicates `_ConvBnAct.backward` and `_ConvBnActCout1.backward` each spelled out
    (join eligibility, the abs-max slot, dy as planes, dy as planes beside fp32) are written out below as they stood, as the specification.
  * `ops._caps` -- the per-descriptor capability record -- must hold what the library answers for every descriptor of tests/golden/conv_routes.json,
    and follow VIAI_WGRAD_PATCH_S2 (which the library reads per call).
"""
import itertools

import pytest

from test_conv_routes_cpu import ROWS, _cin1_without_kernel, lib  # noqa: F401  (lib: the fixture)

ACT_NONE, ACT_RELU, ACT_LRELU, ACT_SIGMOID = 0, 1, 2, 3
P16_OK_DGRAD_DY, P16_OK_WGRAD_DY = 2, 4
BOOLS = (False, True)


def spec_conv_bn_act(f16d, f16w, pm, need_x, need_w, need_b, has_bias, training, act, tail, Cout, P16, F16_BACKWARD, JOIN_FUSED):
    """_ConvBnAct.backward of a BatchNorm layer before ops._dy_form: (abs-max slot taken, which BatchNorm-backward pass ran)"""
    join = None
    if tail == "res" and act == ACT_RELU and JOIN_FUSED and P16 and F16_BACKWARD and Cout % 32 == 0 and (need_x or need_w):
        pm_, f16d_, f16w_ = pm, f16d, f16w
        # (exactly the layers whose dy the plain path below would write as planes: same condition)
        if ((f16d_ and need_x) or (f16w_ and need_w)) and (not need_x or (f16d_ and pm_ & P16_OK_DGRAD_DY)) and (not need_w or (f16w_ and pm_ & P16_OK_WGRAD_DY)) \
                and not (need_b and has_bias and not training):
            join = True
            act = ACT_NONE
    if tail == "res" and join is None:
        act = ACT_NONE                      # the activation's gradient was taken in front of the BatchNorm backward
    amax = True if (F16_BACKWARD and ((f16d and need_x) or (f16w and need_w))) else None
    dy_p16 = (P16 and amax is not None and Cout % 32 == 0 and act != ACT_SIGMOID and tail in (None, "up", "res")
              and (need_x or need_w) and (not need_x or (f16d and pm & P16_OK_DGRAD_DY)) and (not need_w or (f16w and pm & P16_OK_WGRAD_DY))
              and not (need_b and has_bias and not training))
    dy_tw = (not dy_p16 and P16 and amax is not None and Cout % 32 == 0 and act != ACT_SIGMOID and tail in (None, "up", "res")
             and need_x and need_w and f16w and bool(pm & P16_OK_WGRAD_DY) and not (need_b and has_bias and not training))
    if dy_tw:
        form = "twin"
    elif join is not None:
        assert dy_p16, "the fused join pass was chosen for a layer whose dy is not written as planes"
        form = "join"
    elif dy_p16:
        form = "planes"
    elif tail == "pool":
        form = "pool"
    else:
        form = "plain"
    return amax is not None, form


def spec_pair(f16d, f16w, pm, need_x, need_x2, need_w1, need_b1, has_bias, training, act, Cmid, P16, F16_BACKWARD):
    """_ConvBnActCout1.backward before ops._dy_form: (abs-max slot taken, dy written as planes)"""
    amax = True if (F16_BACKWARD and ((f16d and (need_x or need_x2)) or (f16w and need_w1))) else None
    want_dy = need_x or need_x2 or need_w1 or (need_b1 and has_bias)
    nx = need_x or need_x2
    dy_p16 = (P16 and want_dy and amax is not None and Cmid % 32 == 0 and act != ACT_SIGMOID and (nx or need_w1)
              and (not nx or (f16d and pm & P16_OK_DGRAD_DY)) and (not need_w1 or (f16w and pm & P16_OK_WGRAD_DY))
              and not (need_b1 and has_bias and not training))
    return amax is not None, bool(dy_p16)


def _masks():
    # the two dy bits in every combination, with the x / linear-tile bits around them set or clear (they must not matter)
    return [m | other for m in (0, P16_OK_DGRAD_DY, P16_OK_WGRAD_DY, P16_OK_DGRAD_DY | P16_OK_WGRAD_DY) for other in (0, 1 | 8 | 16)]


def test_dy_form_agrees_with_the_expressions_it_replaced_on_every_input():
    from viai_amd import ops
    assert (ops.ACT_NONE, ops.ACT_RELU, ops.ACT_LRELU, ops.ACT_SIGMOID) == (ACT_NONE, ACT_RELU, ACT_LRELU, ACT_SIGMOID)
    assert (ops.P16_OK_DGRAD_DY, ops.P16_OK_WGRAD_DY) == (P16_OK_DGRAD_DY, P16_OK_WGRAD_DY)
    names = {ops.DY_PLAIN: "plain", ops.DY_PLANES: "planes", ops.DY_TWIN: "twin", ops.DY_JOIN: "join", ops.DY_POOL: "pool"}
    assert len(names) == 5
    rows, seen = 0, set()
    for pm, f16d, f16w in itertools.product(_masks(), BOOLS, BOOLS):
        caps = ops.Caps(fwd_f16=True, dgrad_f16=f16d, wgrad_f16=f16w, cin1_bn=False, p16=pm)
        for need_x, need_w, need_b, has_bias, training, act, tail, Cout, P16, F16B, JOIN in itertools.product(
                BOOLS, BOOLS, BOOLS, BOOLS, BOOLS, (ACT_NONE, ACT_RELU, ACT_LRELU, ACT_SIGMOID), (None, "up", "res", "pool"), (64, 48), BOOLS, BOOLS, BOOLS):
            want = spec_conv_bn_act(f16d, f16w, pm, need_x, need_w, need_b, has_bias, training, act, tail, Cout, P16, F16B, JOIN)
            amax, form = ops._dy_form(caps, need_x, need_w, need_b, act, tail, has_bias, training, Cout, P16, F16B, JOIN)
            assert (amax, names[form]) == want, (caps, need_x, need_w, need_b, has_bias, training, act, tail, Cout, P16, F16B, JOIN)
            seen.add(want[1])
            rows += 1
    assert rows == 8 * 4 * 2 ** 5 * 4 * 4 * 2 * 2 ** 3 and seen == set(names.values())


def test_dy_form_agrees_with_the_pair_on_every_input():
    """the Cout = 1 pair passes need_x or need_x2 as its data gradient and no tail, and writes planes or fp32: never the twin"""
    from viai_amd import ops
    rows, seen = 0, set()
    for pm, f16d, f16w in itertools.product(_masks(), BOOLS, BOOLS):
        caps = ops.Caps(fwd_f16=True, dgrad_f16=f16d, wgrad_f16=f16w, cin1_bn=False, p16=pm)
        for need_x, need_x2, need_w1, need_b1, has_bias, training, act, Cmid, P16, F16B, JOIN in itertools.product(
                BOOLS, BOOLS, BOOLS, BOOLS, BOOLS, BOOLS, (ACT_NONE, ACT_RELU, ACT_LRELU, ACT_SIGMOID), (64, 48), BOOLS, BOOLS, BOOLS):
            want = spec_pair(f16d, f16w, pm, need_x, need_x2, need_w1, need_b1, has_bias, training, act, Cmid, P16, F16B)
            amax, form = ops._dy_form(caps, need_x or need_x2, need_w1, need_b1, act, None, has_bias, training, Cmid, P16, F16B, JOIN)
            assert (amax, form == ops.DY_PLANES) == want, (caps, need_x, need_x2, need_w1, need_b1, has_bias, training, act, Cmid, P16, F16B, JOIN)
            assert form in (ops.DY_PLAIN, ops.DY_PLANES, ops.DY_TWIN)
            seen.add(want)
            rows += 1
    assert rows == 8 * 4 * 2 ** 6 * 4 * 2 * 2 ** 3 and len(seen) == 3          # (planes without the slot does not exist)


def _valid_rows():
    return [r for r in ROWS if not _cin1_without_kernel(r[0])]


def test_caps_hold_what_the_library_answered(lib, monkeypatch):  # noqa: F811
    from viai_amd import ops
    monkeypatch.delenv("VIAI_WGRAD_PATCH_S2", raising=False)
    rows = _valid_rows()
    assert len(rows) >= 150
    for r in rows:
        d = ops.conv_desc(*r[0])
        caps = ops._caps(d)
        assert [int(caps.fwd_f16), int(caps.dgrad_f16), int(caps.wgrad_f16), caps.p16] == r[5:9], r[0]
        assert caps.cin1_bn == bool(lib.viai_conv2d_cin1_bn_ok(d["ref"])) and ops.p16_mask(d) == caps.p16
        assert ops._caps(d) is caps                                           # asked once
        for k in ("ref", "OH", "OW", "N", "nblk", "rows", "tiles", "packed", "ws_floats"):
            assert k in d


def test_caps_follow_the_stride2_patch_switch(lib, monkeypatch):  # noqa: F811
    """the library reads VIAI_WGRAD_PATCH_S2 per call: the record made with the switch set holds the answers given with the switch set -- the
    weight-gradient answer like the mask -- whatever was recorded for the descriptor before"""
    from viai_amd import ops
    monkeypatch.delenv("VIAI_WGRAD_PATCH_S2", raising=False)
    before = {tuple(r[0]): ops._caps(ops.conv_desc(*r[0])) for r in _valid_rows()}
    monkeypatch.setenv("VIAI_WGRAD_PATCH_S2", "0")
    for key, old in before.items():
        d = ops.conv_desc(*key)
        caps = ops._caps(d)
        assert caps is not old
        assert caps.wgrad_f16 == bool(lib.viai_conv2d_wgrad_f16_ok(d["ref"])) and caps.p16 == lib.viai_conv2d_p16_ok(d["ref"]) == ops.p16_mask(d), key
        assert (caps.fwd_f16, caps.dgrad_f16, caps.cin1_bn) == (old.fwd_f16, old.dgrad_f16, old.cin1_bn), key
    monkeypatch.delenv("VIAI_WGRAD_PATCH_S2")
    for key, old in before.items():
        assert ops._caps(ops.conv_desc(*key)) is old                          # and back: the first record is still there
