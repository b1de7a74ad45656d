"""Waveform inpainting, the parts that need no GPU: the new C symbols and their types, `_synth_form` with its new argument, the argument checks of
a masked `incremental_forward` call and of `inpaint_waveform`, `gaps_from_mask` against `make_time_mask`."""
import ctypes as C
import itertools
import os

import pytest
import torch

NEW = {
    "viai_wavenet_synth_step_forced": 3,
    "viai_wavenet_synth_run_forced": 5,
    "viai_wn_window_gather": 16,
    "viai_wn_splice": 11,
}


def make_net(onehot=False):
    from viai_amd.wavenet import WaveNet
    torch.manual_seed(5)
    return WaveNet(out_channels=8 if onehot else 30, layers=4, stacks=2, residual_channels=8, gate_channels=8, skip_out_channels=8, cin_channels=4,
                   upsample_scales=(2, 2), scalar_input=not onehot, weight_normalization=False).eval()


def test_new_symbols_are_exported_and_typed():
    from viai_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    assert lib.viai_abi_version() == 20 == _lib.ABI_VERSION
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "viai_hip.h")) as f:
        header = f.read()
    for name, nargs in NEW.items():
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == nargs, name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == list(args)
        assert ("int %s(" % name) in header
    assert _lib.SIGNATURES["viai_wavenet_synth_run_forced"][1][0] == C.POINTER(_lib.WnSynth)
    # the existing entry points keep their signatures
    assert _lib.SIGNATURES["viai_wavenet_synth_run"] == (C.c_int, [C.POINTER(_lib.WnSynth), C.c_int, C.c_int, C.c_void_p])
    assert _lib.SIGNATURES["viai_wavenet_synth_step"] == (C.c_int, [C.POINTER(_lib.WnSynth), C.c_void_p])


def test_host_side_refusals_of_the_new_entry_points():
    """arguments the host checks before any launch: no device is touched"""
    from viai_amd import _lib
    lib = _lib.load()
    inval = 1                                                            # hipErrorInvalidValue
    one = 16                                                             # stands for a device pointer that is never followed
    assert lib.viai_wn_window_gather(one, None, one, one, one, one, None, one, one, 1, 8, 4, 2, 6, 127, None) == inval        # cin % 4
    assert lib.viai_wn_window_gather(None, None, None, one, one, None, None, None, one, 1, 8, 4, 2, 4, 127, None) == inval    # no input
    assert lib.viai_wn_window_gather(one, None, None, one, one, None, None, None, one, 1, 8, 4, 2, 4, 127, None) == inval     # no x_out
    assert lib.viai_wn_splice(one, one, one, one, one, 1, 8, 4, 2, -1, None) == inval                                        # fade < 0
    st = _lib.WnSynth()
    st.B, st.C, st.G, st.S, st.cin, st.n_layers, st.out_ch, st.T, st.n_test = 1, 8, 8, 8, 4, 1, 30, 6, 3
    assert lib.viai_wavenet_synth_run_forced(C.byref(st), one, 0, 1, None) == inval                                          # n_test != T


def test_synth_form_with_the_new_argument():
    from viai_amd.wavenet_synth import _synth_form

    def outcome(*args, **kw):
        try:
            return _synth_form(*args, **kw)
        except Exception as e:
            return type(e), str(e)
    bools = (False, True)
    for args in itertools.product(bools, bools, bools, bools, bools, bools, range(34), (1, 2, 3, 100)):
        plain = outcome(*args)
        assert outcome(*args, masked=False) == plain, args
        # a masked call is the call the pipelined form is not offered to
        use_graph, fuse, pipe_env, pipe_ok, cat_ok, cat, B, T = args
        assert outcome(*args, masked=True) == outcome(use_graph, fuse, pipe_env, False, cat_ok, cat, B, T), args
        assert outcome(*args, masked=True) != "pipe"


@pytest.mark.parametrize("onehot", [False, True])
def test_resolve_inputs_refuses_a_mask_without_matching_test_inputs(onehot):
    from viai_amd.wavenet_synth import _resolve_inputs
    net = make_net(onehot)
    B, T, K = 2, 6, net.out_channels
    full = torch.nn.functional.one_hot(torch.arange(B * T).reshape(B, T) % K, K).float() if onehot else torch.rand(B, 1, T)
    short = full[:, :4] if onehot else full[:, :, :4]
    u = torch.rand(B, T) if onehot else (torch.rand(B, T, 10), torch.rand(B, T))
    mask = torch.zeros(B, T, dtype=torch.bool)
    mask[0, 2:4] = True

    def call(test_inputs, forced):
        return _resolve_inputs(net, None, None, None, T, test_inputs, True, True, u, False, False, "auto", forced)
    with pytest.raises(ValueError, match="needs test_inputs"):
        call(None, mask)
    with pytest.raises(ValueError, match="exactly its length"):
        call(short, mask)
    for bad in (mask[:1], mask.unsqueeze(-1), mask.float(), torch.zeros(B + 1, T, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            call(full, bad)
    inp = call(full, mask)
    assert inp.T == T and inp.forced.dtype == torch.uint8 and torch.equal(inp.forced.bool(), mask)
    assert call(full, mask.to(torch.uint8)).forced.dtype == torch.uint8
    assert call(full, None).forced is None
    if onehot:
        junk = full.clone()
        junk[1, 5] = 0.25                                                # a row the mask does not force may hold anything: still the class form
        assert call(junk, mask).tcls is not None and call(junk, None).tcls is None
        cls = full.argmax(-1)
        got = call(cls, mask)                                            # integer classes: the class form without a one-hot tensor
        assert got.tin is None and torch.equal(got.tcls.long(), cls)


def test_inpaint_waveform_checks_its_arguments_before_the_device():
    from viai_amd.wavenet import inpaint_waveform
    net = make_net()
    c = torch.rand(2, 4, 10)
    with pytest.raises(ValueError, match="frames"):
        inpaint_waveform(net, torch.zeros(2, 41), c, [2, 3], [1, 1])    # n != frames * hop (hop = 4)
    with pytest.raises(ValueError, match="frames"):
        inpaint_waveform(net, torch.zeros(2, 36), c, [2, 3], [1, 1])
    with pytest.raises(ValueError, match="inside the clip"):
        inpaint_waveform(net, torch.zeros(2, 40), c, [2, 9], [1, 2])
    with pytest.raises(ValueError, match="per stream"):
        inpaint_waveform(net, torch.zeros(2, 40), c, [2, 3, 4], [1, 1, 1])
    with pytest.raises(ValueError):
        inpaint_waveform(net, torch.zeros(2, 40), None, [2, 3], [1, 1])


def test_gaps_from_mask_round_trips_make_time_mask():
    from viai_amd.model import make_time_mask
    from viai_amd.wavenet import gaps_from_mask
    gen = torch.Generator().manual_seed(3)
    for frames, blank in ((208, 52), (16, 4), (9, 1)):
        mask = make_time_mask(8, frames, blank, generator=gen)
        g0, ln = gaps_from_mask(mask)
        assert g0.dtype == torch.int64 and tuple(g0.shape) == (8,) and torch.equal(ln, torch.full((8,), blank))
        ar = torch.arange(frames)[None, :]
        rebuilt = ((ar < g0[:, None]) | (ar >= (g0 + ln)[:, None])).float().view(8, 1, 1, frames)
        assert torch.equal(rebuilt, mask)
    two = torch.ones(1, 1, 1, 12)
    two[..., 2:4] = 0
    two[..., 7] = 0
    with pytest.raises(ValueError, match="more than one gap"):
        gaps_from_mask(two)
    g0, ln = gaps_from_mask(torch.ones(2, 1, 1, 5))
    assert g0.tolist() == [0, 0] and ln.tolist() == [0, 0]
