"""CPU: the host side of the WaveNet batch assembly (viai_amd.vocoder_batch): the crop plan against the reference's own draws and lengths
(tests/golden/vocoder_batch.npz, tools/make_vocoder_batch_golden.py), the new C-ABI symbol and its host refusals, loud failures."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = "viai_voc_collate"
CASES = ("no_crop", "crop", "exact_is_not_cropped", "one_window_short", "steps_not_divisible", "max_time_sec", "raw", "speaker_ids", "hop256")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "vocoder_batch.npz"))


@pytest.fixture(scope="module")
def lib():
    from viai_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def settings(g, name):
    hop, D, mts, sr, K, seed = (int(v) for v in g[name + ".settings"])
    sec = float(g[name + ".max_time_sec"])
    return dict(hop=hop, D=D, max_time_steps=None if mts < 0 else mts, max_time_sec=None if np.isnan(sec) else sec, sample_rate=sr, K=K, seed=seed)


def test_crop_plan_reproduces_the_reference(golden):
    from viai_amd.vocoder_batch import crop_plan
    assert tuple(golden["names"].tolist()) == CASES
    for name in CASES:
        s = settings(golden, name)
        n = golden[name + ".n_frames"].tolist()
        want_starts, lengths = golden[name + ".starts"].tolist(), golden[name + ".input_lengths"].tolist()
        starts, frames = crop_plan(n, s["hop"], s["max_time_steps"], s["max_time_sec"], s["sample_rate"], rng=np.random.RandomState(s["seed"]))
        assert starts == want_starts and [f * s["hop"] for f in frames] == lengths, name
        # the draws themselves, in the order the reference made them: one per cropped row, high bound n - L exclusive
        draws = golden[name + ".draws"].tolist()
        assert [[a - f, st] for st, a, f in zip(starts, n, frames) if f < a] == draws, name
        # injected starts give the same plan and draw nothing
        assert crop_plan(n, s["hop"], s["max_time_steps"], s["max_time_sec"], s["sample_rate"], starts=want_starts) == (starts, frames), name
    # the branches by name
    plan = lambda name: (golden[name + ".n_frames"].tolist(), golden[name + ".starts"].tolist(), golden[name + ".input_lengths"].tolist())
    assert plan("no_crop")[1:] == ([0, 0, 0], [12, 28, 20])
    n, st, ln = plan("crop")
    assert len({v for v in st if v > 0}) >= 2 and ln == [24, 20, 24, 24, 24] and n[4] * 4 == 24 and st[4] == 0
    n, st, ln = plan("exact_is_not_cropped")
    assert n[0] * 4 == 24 == ln[0] and st[0] == 0 and golden["exact_is_not_cropped.draws"].shape[0] == 1
    n, st, ln = plan("one_window_short")
    assert n[0] - 6 == 1 and st[0] == 0 and [1, 0] in golden["one_window_short.draws"].tolist()
    assert settings(golden, "steps_not_divisible")["max_time_steps"] % 4 != 0 and plan("steps_not_divisible")[2] == [24, 16, 24]
    assert settings(golden, "max_time_sec")["max_time_sec"] is not None and plan("max_time_sec")[2] == [24, 24, 24]
    for name in ("crop", "steps_not_divisible", "max_time_sec", "hop256"):                  # the order of the draws is pinned
        assert len({v for v in plan(name)[1] if v > 0}) >= 2, name


def test_a_row_one_window_longer_always_starts_at_zero():
    from viai_amd.vocoder_batch import crop_plan
    for seed in range(20):
        starts, frames = crop_plan([7, 6, 8], 4, max_time_steps=24, rng=np.random.RandomState(seed))
        assert starts[0] == 0 and starts[1] == 0 and starts[2] in (0, 1) and frames == [6, 6, 6]          # 2 = n - L is never drawn
    assert crop_plan([5, 9], 256) == ([0, 0], [5, 9])                                                 # no crop configured
    assert crop_plan([5, 9], 256, max_time_steps=100, max_time_sec=1.0, sample_rate=2560, starts=[0, 0]) == ([0, 0], [5, 9])      # sec wins: L = 10


def test_crop_plan_refusals():
    from viai_amd.vocoder_batch import crop_plan
    for args, kw in ((([], 4), {}), (([3, 0], 4), {}), (([3, -1], 4), {}), (([3], 0), {}),
                     (([3], 4), dict(max_time_steps=3)), (([3], 4), dict(max_time_sec=0.0001)),          # L == 0
                     (([8, 9], 4), dict(max_time_steps=24, starts=[0])),                                 # one start per row
                     (([8, 9], 4), dict(max_time_steps=24, starts=[3, 0])),                              # 0 <= s <= n - L = 2
                     (([8, 9], 4), dict(max_time_steps=24, starts=[-1, 0])),
                     (([8, 5], 4), dict(max_time_steps=24, starts=[0, 1])),                              # an uncropped row starts at 0
                     (([8, 5], 4), dict(starts=[1, 0]))):
        with pytest.raises(ValueError):
            crop_plan(*args, **kw)
    assert crop_plan([8, 9], 4, max_time_steps=24, starts=[2, 3]) == ([2, 3], [6, 6])                  # n - L itself is a valid injected start


def test_new_symbol_is_exported_declared_and_bound(lib):
    from viai_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "viai_hip.h")).read(), flags=re.S)
    assert hasattr(lib, NEW) and NEW in _lib.SIGNATURES and re.search(r"\b%s\s*\(" % NEW, text)
    assert len(_lib.SIGNATURES[NEW][1]) == 16
    assert lib.viai_abi_version() == 20 == _lib.ABI_VERSION
    assert "vocoder_batch.hip" in open(os.path.join(ROOT, "vision-infused-audio-inpainter-viai_amd", "csrc", "Makefile")).read()
    assert "data_loader_utils.py:209-319" in open(os.path.join(ROOT, "include", "viai_hip.h")).read()


def test_host_refusals_need_no_device(lib):
    buf = C.create_string_buffer(64)
    p = C.addressof(buf)                                                    # never dereferenced: every call below is refused on the host

    def collate(sig=p, mel=p, start=p, frames=p, B=2, hop=256, D=80, mode=0, K=256, T=1280, L=5, y=p, classes=p, x=p, c=p):
        return lib.viai_voc_collate(sig, mel, start, frames, B, hop, D, mode, K, T, L, y, classes, x, c, 0)
    for kw in (dict(sig=0), dict(start=0), dict(frames=0), dict(y=0), dict(B=0), dict(B=-1), dict(B=65536), dict(hop=0), dict(hop=-4), dict(mode=3),
               dict(mode=-1), dict(K=1), dict(K=0), dict(K=254), dict(K=6), dict(D=0), dict(D=-1), dict(mel=0), dict(c=0), dict(T=255, L=0),
               dict(T=0, L=0), dict(T=1281), dict(T=1300, L=5), dict(L=4), dict(L=6), dict(T=2 ** 31, L=2 ** 23), dict(hop=1, T=2 ** 31, L=2 ** 31 - 1)):
        assert collate(**kw) != 0, kw
    assert collate(mode=2, K=1, x=p) != 0 and collate(mode=1, K=6, x=p) != 0                      # K % 4 with x given, whatever the mode


def test_bad_arguments_raise_before_the_library_is_loaded(monkeypatch):
    from viai_amd import _lib, vocoder_batch as VB

    def no_load():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", no_load)
    for kw in (dict(input_type="ulaw"), dict(quantize_channels=1), dict(hop=0), dict(max_time_steps=100), dict(max_time_sec=0.001), dict(pad_to=0),
               dict(one_hot=True, quantize_channels=6), dict(one_hot=True, input_type="raw"), dict(upsample_conditional_features=False)):
        with pytest.raises(ValueError):
            VB.VocoderBatcher(**kw)
    vb = VB.VocoderBatcher()
    assert (vb.hop, vb.sample_rate, vb.K, vb.mode, vb.one_hot, vb.pad_to) == (256, 16000, 256, 0, False, None)
    sig, mel = torch.zeros(3 * 256, dtype=torch.int32), torch.zeros(3, 80)
    with pytest.raises(_lib.ViaiLibraryError, match="GPU only; no CPU fallback"):
        vb([(sig, mel)])
    with pytest.raises(_lib.ViaiLibraryError, match="GPU only; no CPU fallback"):
        VB.VocoderBatcher(input_type="raw")([(sig.float(), None)])
    with pytest.raises(ValueError):
        vb([])
    with pytest.raises(ValueError):
        vb([(sig.tolist(), mel)])
    # (the checks behind the device check -- dtype, contiguity, lengths, one D -- need GPU tensors: test_vocoder_batch_gpu.py)
    with pytest.raises(ValueError):
        vb([(sig, mel), (sig, None)])                                       # a mel for every row or for none
    with pytest.raises(ValueError):
        VB.VocoderBatcher(max_time_steps=1024)([(sig, None)])              # the branch without local conditioning crops on the sample grid: not ported


def test_vocoder_batch_is_a_submodule_only():
    import viai_amd
    import viai_amd.vocoder_batch  # noqa: F401
    with pytest.raises(AttributeError):
        viai_amd.VocoderBatcher
