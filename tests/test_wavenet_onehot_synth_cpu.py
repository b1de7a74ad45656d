"""No GPU: what sample-by-sample synthesis of the one-hot (softmax) WaveNet rests on -- the host-side descriptor query of the C ABI, the
conditions on tests/golden/wavenet_onehot_synth.npz that make the GPU tests fair (tools/make_goldens.py wavenet_onehot_synth_goldens asserts
the same when it writes the file), and the refusal of softmax=False / quantize=True before any device work."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import viai_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from viai_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def descriptor(B=1, K=256, **kw):
    from viai_amd._lib import WnSynth
    st = WnSynth()
    st.B, st.C, st.G, st.S, st.cin, st.n_layers, st.out_ch, st.T = B, 64, 64, 32, 80, 4, K, 16
    st.categorical, st.cat_softmax, st.cat_quantize, st.init_class = 1, 1, 1, 127 if K > 127 else 0
    for k, v in kw.items():
        setattr(st, k, v)
    return st


def test_categorical_descriptor_query(lib):
    ok = lambda st: lib.viai_wn_categorical_ok(C.byref(st))
    assert ok(descriptor(K=256)) == 1 and ok(descriptor(K=64)) == 1
    for B in (2, 4, 8):
        assert ok(descriptor(B=B)) == 1
    assert ok(descriptor(K=260)) == 0            # more classes than the sampler's block has threads
    assert ok(descriptor(K=254)) == 0            # rows of the first-conv weight are read 16 bytes at a time
    assert ok(descriptor(B=3)) == 0
    assert ok(descriptor(cat_softmax=0)) == 0    # quantize without softmax: the reference raises (wavenet.py:351-354)
    assert ok(descriptor(cat_softmax=0, cat_quantize=0)) == 1 and ok(descriptor(cat_quantize=0)) == 1
    assert ok(descriptor(categorical=0)) == 0    # a mixture-of-logistics descriptor is not a categorical one
    assert ok(descriptor(init_class=256)) == 0


def test_pipelined_form_refuses_a_categorical_descriptor(lib):
    """csrc/wavenet_pipe.hip stays mixture-of-logistics only: the reference-size dimensions with the categorical flag set are refused on
    the flag alone (the layer array is never looked at: it is NULL here)."""
    st = descriptor(B=8, K=30, C=512, G=512, S=256, n_layers=24)
    assert lib.viai_wn_pipe_ok(C.byref(st)) == 0


def test_fixture_conditions():
    """the sampled classes follow from the stored probabilities and the closed-form uniforms by the inverse-CDF draw; every draw keeps the stored
    distance from the CDF's edges (>= 1e-4 small / >= 3e-5 deep); the free-running probabilities differ from the teacher-forced ones by >= 1e-2."""
    gold = np.load(os.path.join(ROOT, "tests", "golden", "wavenet_onehot_synth.npz"))
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "wavenet_onehot_synth.npz")) <= 523767
    for name, need in (("small", 1e-4), ("deep", 3e-5)):
        B, T, K, stride, utag = (int(v) for v in gold[name + ".meta"])
        assert (B, K) == (2, 256) and T == (64 if name == "small" else 160)
        u = O.cf_uniform("wnos.%s.u%d" % (name, utag), (1, T), 0, 1).numpy().reshape(T).astype(np.float64)
        assert u.min() >= 0.0 and u.max() < 1.0
        cls, margins, p = gold[name + ".classes"], gold[name + ".margins"], gold[name + ".p_samp"].astype(np.float64)
        assert cls.shape == (T,) and margins.shape == (T,) and p.shape == (len(range(0, T, stride)), K)
        assert margins.min() >= need, margins.min()
        cdf = np.cumsum(p, axis=1)
        cdf /= cdf[:, -1:]
        us = u[::stride]
        assert np.array_equal(np.minimum((cdf <= us[:, None]).sum(1), K - 1), cls[::stride])
        assert np.allclose(np.abs(cdf - us[:, None]).min(1), margins[::stride], rtol=0, atol=1e-12)
        p_tf, p_free = gold[name + ".p_tf"].astype(np.float64), gold[name + ".p_free"].astype(np.float64)
        assert p_tf.shape == p_free.shape == (B, K, len(range(0, T, stride)))
        assert np.allclose(p_tf.sum(1), 1.0, atol=1e-5) and np.allclose(p_free.sum(1), 1.0, atol=1e-5)
        dist = np.linalg.norm(p_free - p_tf) / np.linalg.norm(p_tf)
        assert dist >= 1e-2 and float(gold[name + ".feedback_dist"]) >= 1e-2, dist
        assert np.array_equal(p_tf[:, :, 0], p_free[:, :, 0])          # step 0 is teacher-forced in both runs
        # the stored logits are the stored probabilities' logits
        steps = gold[name + ".logit_steps"]
        keep = [i for i, t in enumerate(steps) if t % stride == 0]
        sm = torch.softmax(torch.from_numpy(gold[name + ".l_tf"]).double(), 1).numpy()
        assert np.abs(sm[:, :, keep] - p_tf[:, :, [int(steps[i]) // stride for i in keep]]).max() < 1e-6


def test_quantize_without_softmax_is_refused_before_the_library_is_loaded(monkeypatch):
    from viai_amd import _lib
    from viai_amd.wavenet import WaveNet

    def no_load():
        raise AssertionError("the library was asked for before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_load)
    net = WaveNet(out_channels=8, layers=2, stacks=1, residual_channels=8, gate_channels=8, skip_out_channels=8, cin_channels=-1,
                  upsample_conditional_features=False, scalar_input=False).eval()
    with pytest.raises(ValueError):
        net.incremental_forward(None, T=4, softmax=False, quantize=True)
