"""No GPU: what training the one-hot (softmax) WaveNet from class indices rests on -- the four entry points of ABI 20 in the built library and
their ctypes signatures, the fixture tests/golden/wavenet_onehot_train.npz restated through the oracle in fp64, and the mu-law check vectors
the GPU test quantises (built here in fp64, with their distance from a rounding edge)."""
import os

import numpy as np
import pytest
import torch

from oracle import viai_oracle as O
from oracle import wavenet_oracle as W

NEW_ENTRY_POINTS = ("viai_masked_ce_loss", "viai_class_embed_fwd", "viai_class_embed_bwd", "viai_mulaw_quantize")


@pytest.fixture(scope="module")
def lib():
    from viai_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def mulaw_vectors(mu=255):
    """x_k = decode(k + 0.5), the centre of class k's interval, for k = 0 .. mu - 1, then -1, 0, 1; the value (y + 1) / 2 * mu the
    quantiser truncates, in fp64; the expected classes"""
    k = np.arange(mu, dtype=np.float64)
    y = 2.0 * (k + 0.5) / mu - 1.0
    x = np.sign(y) * np.expm1(np.abs(y) * np.log1p(mu)) / mu
    x = np.concatenate([x, [-1.0, 0.0, 1.0]])
    pre = (np.sign(x) * np.log1p(mu * np.abs(x)) / np.log1p(mu) + 1.0) / 2.0 * mu
    want = np.concatenate([np.arange(mu), [0, mu // 2, mu]]).astype(np.int64)
    return x, pre, want


def test_library_exports_and_types_the_new_entry_points(lib):
    from viai_amd import _lib
    for n in NEW_ENTRY_POINTS + ("viai_class_embed_bwd_segments",):
        assert hasattr(lib, n), "libviai_hip.so does not export %s" % n
        assert n in _lib.SIGNATURES, "no ctypes signature for %s" % n
        assert getattr(lib, n).argtypes == _lib.SIGNATURES[n][1]
    # the row segments of the weight gradient: whole 2048-row chunks, at least one
    assert [lib.viai_class_embed_bwd_segments(r) for r in (1, 2048, 2049, 32768, 1 << 24)] == [1, 1, 2, 16, 64]
    # shape conditions are refused on the host, before any launch: K % 4, pitch < K, shift >= T, C % 4, C > 1024
    assert lib.viai_masked_ce_loss(0, 0, 0, 0, 0, 0, 0, 1, 8, 254, 256, 0, 0) != 0
    assert lib.viai_masked_ce_loss(0, 0, 0, 0, 0, 0, 0, 1, 8, 256, 252, 0, 0) != 0
    assert lib.viai_masked_ce_loss(0, 0, 0, 0, 0, 0, 0, 1, 8, 256, 256, 8, 0) != 0
    assert lib.viai_class_embed_fwd(0, 0, 0, 0, 0, 16, 256, 30, 0) != 0
    assert lib.viai_class_embed_bwd(0, 0, 0, 0, 0, 16, 256, 2048, 0) != 0


def test_abi_version_is_20(lib):
    from viai_amd import _lib
    assert lib.viai_abi_version() == 20 == _lib.ABI_VERSION


def test_python_surface_exists():
    from viai_amd import losses, wavenet
    assert losses.MaskedCrossEntropyLoss is wavenet.MaskedCrossEntropyLoss
    for n in ("masked_cross_entropy", "mulaw_quantize", "mulaw_decode"):
        assert callable(getattr(wavenet, n))
    with pytest.raises(RuntimeError, match="Should provide either lengths or mask"):
        wavenet.MaskedCrossEntropyLoss()(torch.zeros(1, 4, 3), torch.zeros(1, 3, 1, dtype=torch.long))


def test_fixture_is_self_consistent(golden_dir):
    """the oracle forward + an fp64 masked cross-entropy on the stored inputs reproduce the stored loss, and the mask leaves rows out"""
    gold = np.load(golden_dir + "/wavenet_onehot_train.npz")
    cfg = W.WNConfigOneHot
    B, T, K = [int(v) for v in gold["small.meta"]]
    assert (B, T, K) == (2, 64, cfg.out_channels)
    idx = torch.from_numpy(gold["small.idx"])
    assert torch.equal(idx, (O.cf_uniform("wnot.small.idx", (B, T), 0, 1) * K).long().clamp(max=K - 1))
    lengths = torch.from_numpy(gold["small.lengths"])
    assert lengths.tolist() == [T - 1, T - 15]
    mask = (torch.arange(T - 1).unsqueeze(0) < lengths.unsqueeze(1)).double()
    assert 0 < mask.sum().item() < B * (T - 1)
    x = torch.nn.functional.one_hot(idx, K).float().transpose(1, 2).contiguous()
    c = O.cf_uniform("wnot.small.c", (B, cfg.cin_channels, T // 16), 0, 1)
    with torch.no_grad():
        yh = W.wavenet_forward(W.wavenet_state(cfg), x, c, cfg)
    assert np.linalg.norm(yh.numpy() - gold["small.yhat"]) < 1e-5 * np.linalg.norm(gold["small.yhat"])
    ce = torch.nn.functional.cross_entropy(yh[:, :, :-1].double(), idx[:, 1:], reduction="none")
    loss = ((ce * mask).sum() / mask.sum()).item()
    assert abs(loss - float(gold["small.loss"])) < 1e-5 * float(gold["small.loss"])
    # the reference-width case: digests only, one stream, the shorter length
    Bf, Tf, Kf = [int(v) for v in gold["full.meta"]]
    assert (Bf, Tf, Kf) == (1, 1024, 256) and gold["full.lengths"].tolist() == [Tf - 15]
    assert all(gold[k].shape == (67,) for k in gold.files if k.startswith("full.g."))
    assert os.path.getsize(golden_dir + "/wavenet_onehot_train.npz") < (1 << 20)


def test_mulaw_check_vectors_sit_mid_interval():
    """every check vector's pre-truncation value is 0.5 away from an integer (fp64: 1e-12 or less off), so an fp32 kernel needs no
    exclusion for rounding: its error at these points is a few 2^-24 * 255"""
    x, pre, want = mulaw_vectors()
    assert x.shape == (258,) and np.all(np.abs(x) <= 1.0)
    frac = pre[:255] - np.floor(pre[:255])
    assert np.abs(frac - 0.5).max() < 1e-12, np.abs(frac - 0.5).max()
    assert np.array_equal(np.floor(pre[:255]).astype(np.int64), want[:255])
    assert pre[255] == 0.0 and pre[256] == 127.5 and pre[257] == 255.0           # -1, 0, 1: classes 0, 127, 255 (the clamp keeps 255)
    assert want[255:].tolist() == [0, 127, 255]
