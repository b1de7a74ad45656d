"""GPU: the counter-based dropout of the WaveNet residual layers (`viai_dropout`, csrc/dropout.hip) -- the exact Philox stream against a
numpy restatement, dropped elements as a select, in-place use, the mask-free backward, one residual layer against the same layer fed a
hand-dropped input, and the seed / call-counter / state behaviour of both networks in train mode.  Everything here is integer arithmetic and
one fp32 multiply, or the same kernels on the same inputs twice: every comparison is bit for bit."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import viai_oracle as O
from oracle import wavenet_oracle as W

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
LO, S32 = np.uint64(0xFFFFFFFF), np.uint64(32)
P = 0.05


def philox4x32_10(counter, key):
    """tests/test_wavenet_dropout_cpu.py's restatement (checked there against the Random123 known-answer vectors)"""
    c = [np.asarray(v, dtype=np.uint64) & LO for v in counter]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> S32) ^ c[1] ^ np.uint64(k0), p1 & LO, (p0 >> S32) ^ c[3] ^ np.uint64(k1), p0 & LO]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


def keep_mask(n, p, seed, offset, first=0):
    """keep flags of elements first .. n - 1 (first a multiple of 4): element 4 j + k is word k of counter (j lo, j hi, offset lo, offset hi),
    key (seed lo, seed hi); kept iff word >= floor(p * 2^32)"""
    assert first % 4 == 0
    j = np.arange(first // 4, (n + 3) // 4, dtype=np.uint64)
    z = np.zeros_like(j)
    w = philox4x32_10((j & LO, j >> S32, z + np.uint64(offset & 0xFFFFFFFF), z + np.uint64(offset >> 32)), (seed & 0xFFFFFFFF, seed >> 32))
    return np.stack(w, axis=1).reshape(-1)[:n - first] >= np.uint64(int(np.floor(p * 4294967296.0)))


def want_dropout(x32, mask, p):
    return np.where(mask, x32 * np.float32(1 / (1 - p)), np.float32(0))


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def raw_dropout(x, y, p, seed, offset):
    from viai_amd import _lib
    _lib.check(_lib.load().viai_dropout(x.data_ptr(), y.data_ptr(), x.numel(), p, seed, offset, torch.cuda.current_stream().cuda_stream), "viai_dropout")
    return y


# ----------------------------------------------------------------------------- 1. the exact stream
def test_exact_stream():
    """1. mask and values equal the numpy restatement exactly: sizes around the float4 width and with a tail, both key words, both offset
    words; the fixed kept count of the stream the CPU test pins"""
    from viai_amd.wavenet import dropout, dropout_mask
    src = O.cf_uniform("drop.x", (4099,), -2, 2)
    for n in (1, 2, 3, 4, 5, 7, 8, 9, 4096, 4099):
        x = src[:n].cuda()
        x32 = src[:n].numpy()
        for p in (0.05, 0.5):
            for seed in (1234, 2 ** 40 + 3):
                for offset in (0, 1, 2 ** 32 + 5):
                    m = keep_mask(n, p, seed, offset)
                    got = dropout_mask((n,), p, seed, offset)
                    assert got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), m), (n, p, seed, offset)
                    y = dropout(x, p, seed, offset)
                    assert y.data_ptr() != x.data_ptr()
                    assert np.array_equal(y.cpu().numpy().view(np.int32), want_dropout(x32, m, p).view(np.int32)), (n, p, seed, offset)
    assert int(dropout_mask((4096,), 0.05, 1234, 0).sum()) == 3912
    assert dropout_mask((4, 1, 8, 32), 0.05, 1234, 0).shape == (4, 1, 8, 32)
    assert bool(dropout_mask((9,), 0.0, 1234, 0).all())
    assert dropout(x, 0.0, 1234, 0) is x


def test_views_use_the_flat_element_index():
    """1b. the element index is the position in the contiguous tensor: a 4-D shape, a transposed view and a view that starts inside a float4
    give the values of their contiguous copies"""
    from viai_amd.wavenet import dropout
    src = O.cf_uniform("drop.v", (2, 1, 37, 12), -2, 2)
    m = keep_mask(src.numel(), P, 99, 7)
    y = dropout(src.cuda(), P, 99, 7)
    assert y.shape == src.shape and np.array_equal(y.cpu().numpy().reshape(-1).view(np.int32), want_dropout(src.numpy().reshape(-1), m, P).view(np.int32))
    t = src.cuda().transpose(2, 3)
    assert bits_equal(dropout(t, P, 99, 7), dropout(t.contiguous(), P, 99, 7))
    flat = src.reshape(-1).cuda()
    for start in (1, 2, 3):
        v = flat[start:]
        assert v.data_ptr() % 16 != 0
        assert bits_equal(dropout(v, P, 99, 7), dropout(v.clone(), P, 99, 7))


def test_byte_offsets_past_2_gib():
    """1c. 2^29 + 7 elements in place (the byte offset passes 2^31, the grid-stride loop makes many trips): the last 4096 + 7 elements, tail
    included, against numpy; the kept share of the whole within 5 sigma of 1 - p"""
    n = (1 << 29) + 7
    x = torch.ones(n, device="cuda")
    raw_dropout(x, x, P, 1234, 3)
    first = (1 << 29) - 4096
    m = keep_mask(n, P, 1234, 3, first=first)
    assert np.array_equal(x[first:].cpu().numpy().view(np.int32), want_dropout(np.ones(n - first, np.float32), m, P).view(np.int32))
    kept = int(torch.count_nonzero(x))
    thr = math.floor(P * 2 ** 32) / 2 ** 32
    assert abs(kept - n * (1 - thr)) < 5 * math.sqrt(n * thr * (1 - thr)), kept


# ----------------------------------------------------------------------------- 2, 3. select; in place
def test_dropped_elements_are_a_select():
    """2. inf, -inf, NaN and -1 at dropped positions come out as +0.0 (sign bit clear): nothing non-finite leaks through a dropped element"""
    from viai_amd.wavenet import dropout
    n = 4099
    m = keep_mask(n, P, 1234, 7)                                                      # offset 7: element 4097, in the scalar tail, is dropped
    dropped = np.flatnonzero(~m)
    assert len(dropped) >= 8 and dropped[-1] >= 4096                                  # one of them in the scalar tail
    x = torch.ones(n)
    where = list(dropped[:4]) + list(dropped[-4:])
    for i, v in zip(where, [float("inf"), float("-inf"), float("nan"), -1.0] * 2):
        x[i] = v
    y = dropout(x.cuda(), P, 1234, 7)
    assert torch.isfinite(y).all().item()
    assert torch.count_nonzero(bits(y)[torch.from_numpy(dropped).cuda()]).item() == 0  # all bits clear: +0.0
    assert np.array_equal(y.cpu().numpy().view(np.int32), want_dropout(np.ones(n, np.float32), m, P).view(np.int32))


def test_in_place():
    """3. x and y the same pointer: the bits of the out-of-place call"""
    for n in (7, 4099, 300001):
        x = O.cf_uniform("drop.ip.%d" % n, (n,), -2, 2).cuda()
        y = raw_dropout(x, torch.empty_like(x), P, 5, 9)
        z = x.clone()
        raw_dropout(z, z, P, 5, 9)
        assert bits_equal(y, z) and not bits_equal(y, x)


# ----------------------------------------------------------------------------- 4. backward
def test_backward_recomputes_the_mask():
    """4. x.grad is dropout(g) with the same arguments, bit for bit, and the forward allocates its output only: no mask tensor (a bool mask
    would be n bytes; the slack is one 512-byte allocator granule)"""
    from viai_amd.wavenet import dropout
    n = 1000003
    x = O.cf_uniform("drop.bw.x", (n,), -2, 2).cuda().requires_grad_(True)
    g = O.cf_uniform("drop.bw.g", (n,), -2, 2).cuda()
    want = dropout(g, P, 77, 1025)
    del_me = dropout(x.detach(), P, 77, 1025)                                         # warm: code object loaded, nothing lazy left to allocate
    del del_me
    torch.cuda.synchronize()
    # bytes ASKED of the allocator, not the blocks it handed out: a cached block is given whole when a split would leave under 1 MiB, so
    # the block count depends on what earlier tests left in the cache (seen: 4388352 bytes for this output, no second tensor)
    def requested():
        return torch.cuda.memory_stats()["requested_bytes.all.current"]
    before = requested()
    y = dropout(x, P, 77, 1025)
    torch.cuda.synchronize()
    grown = requested() - before
    print("forward grew the allocator by %d bytes for an output of %d" % (grown, 4 * n))
    assert 4 * n <= grown <= 4 * n + 512, grown
    assert y.grad_fn is not None and len(getattr(y.grad_fn, "saved_tensors", ())) == 0
    y.backward(g)
    assert bits_equal(x.grad, want)
    assert bits_equal(y, dropout(x.detach(), P, 77, 1025))


# ----------------------------------------------------------------------------- 5. one residual layer
def test_layer_equals_the_layer_fed_a_hand_dropped_input():
    """5. a ResidualConv1dGLU in train mode with dropout against the same weights without it, fed dropout(x) computed by hand with the layer's
    (seed, offset) while the residual adds the un-dropped x: outputs and the gradients of x and of every parameter, bit for bit"""
    from viai_amd.wavenet import ResidualConv1dGLU, _GLU, add_scale, conv1d_apply, dropout
    cfg = W.WNConfig
    B, T, seed, index, calls = 2, 64, 2 ** 40 + 3, 2, 3

    def layer(p):
        return ResidualConv1dGLU(cfg.residual_channels, cfg.gate_channels, cfg.kernel_size, cfg.skip_out_channels, cfg.cin_channels, -1, p, dilation=2)
    torch.manual_seed(0)
    a = layer(P).cuda().train()
    b = layer(0.0).cuda().train()
    b.load_state_dict(a.state_dict())
    a.layer_index, a._drop_seed, a._drop_calls = index, seed, calls
    x = O.cf_uniform("drop.l.x", (B, 1, T, cfg.residual_channels), -1, 1).cuda()
    c = O.cf_uniform("drop.l.c", (B, 1, T, cfg.cin_channels), 0, 1).cuda()
    g_out = O.cf_uniform("drop.l.go", (B, 1, T, cfg.residual_channels), -1, 1).cuda()
    g_s = O.cf_uniform("drop.l.gs", (B, 1, T, cfg.skip_out_channels), -1, 1).cuda()

    xa = x.clone().requires_grad_(True)
    out_a, s_a = a.forward_nhwc(xa, c)
    assert a._drop_calls == calls + 1
    torch.autograd.backward([out_a, s_a], [g_out, g_s])

    xb = x.clone().requires_grad_(True)
    xd = dropout(xb, P, seed, calls * 1024 + index)
    assert not bits_equal(xd, xb)
    z = _GLU.apply(conv1d_apply(xd, b.conv, causal_crop=True), conv1d_apply(c, b.conv1x1c))
    s_b = conv1d_apply(z, b.conv1x1_skip)
    out_b = add_scale(conv1d_apply(z, b.conv1x1_out), xb, math.sqrt(0.5))             # the residual: the un-dropped input
    torch.autograd.backward([out_b, s_b], [g_out, g_s])

    assert bits_equal(s_a, s_b) and bits_equal(out_a, out_b)
    assert bits_equal(s_a, b.forward_nhwc(xd.detach(), c)[1])                         # and B's own forward on the dropped input gives that s
    assert bits_equal(xa.grad, xb.grad)
    pa, pb = dict(a.named_parameters()), dict(b.named_parameters())
    assert len(pa) == 12
    for k in pa:
        assert pa[k].grad is not None and bits_equal(pa[k].grad, pb[k].grad), k
    # eval mode: no dropout, the call counter stands still
    a.eval()
    with torch.no_grad():
        out_e, s_e = a.forward_nhwc(x, c)
        out_0, s_0 = b.forward_nhwc(x, c)
    assert a._drop_calls == calls + 1 and bits_equal(out_e, out_0) and bits_equal(s_e, s_0)


# ----------------------------------------------------------------------------- 6. the network
def build(cfg, dropout, scalar_input=True):
    from viai_amd.wavenet import WaveNet
    net = WaveNet(out_channels=cfg.out_channels, layers=cfg.layers, stacks=cfg.stacks, residual_channels=cfg.residual_channels,
                  gate_channels=cfg.gate_channels, skip_out_channels=cfg.skip_out_channels, kernel_size=cfg.kernel_size, dropout=dropout,
                  cin_channels=cfg.cin_channels, gin_channels=-1, weight_normalization=True, upsample_conditional_features=True,
                  upsample_scales=list(cfg.upsample_scales), freq_axis_kernel_size=cfg.freq_axis_kernel_size, scalar_input=scalar_input)
    net.load_state_dict(W.wavenet_state(cfg))
    return net.cuda().train()


class Net:
    """the small WaveNet (mixture-of-logistics form, local conditioning) in train mode with dropout = 0.05, its inputs, and one training
    forward + backward as a function"""

    def __init__(self, dropout=P):
        cfg = W.WNConfig
        self.B, self.T, self.cfg = 2, 64, cfg
        self.net = build(cfg, dropout)
        self.x = O.cf_uniform("drop.n.x", (self.B, 1, self.T), -1, 1).cuda()
        self.c = O.cf_uniform("drop.n.c", (self.B, cfg.cin_channels, self.T // 16), 0, 1).cuda()
        self.g = O.cf_uniform("drop.n.g", (self.B, 1, self.T, 32), -1, 1).cuda()

    def step(self):
        """(logits, {name: gradient}) of one forward + backward"""
        self.net.zero_grad(set_to_none=True)
        y = self.net.forward_nhwc(self.x, self.c)
        y.backward(self.g)
        return y.detach().clone(), grads(self.net)


def grads(net):
    """the gradient of every parameter that has one (the last layer's conv1x1_out feeds nothing: the network reads only its skip output)"""
    return {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}


def same(a, b):
    return bits_equal(a[0], b[0]) and a[1].keys() == b[1].keys() and all(bits_equal(a[1][k], b[1][k]) for k in a[1])


@pytest.fixture(scope="module")
def small():
    return Net()


def test_network_same_seed_same_bits(small):
    """6a-c. two passes from seed_dropout(11) agree in every bit of the logits and of every parameter gradient; the next pass without
    reseeding differs (the call counter advanced); so does seed 12"""
    net = small.net
    net.seed_dropout(11)
    first = small.step()
    assert [f._drop_calls for f in net.conv_layers] == [1] * small.cfg.layers
    assert all(torch.isfinite(v).all().item() for v in first[1].values()) and len(first[1]) > 40
    net.seed_dropout(11)
    again = small.step()
    assert same(first, again)
    second = small.step()                                                             # no reseeding: call 1
    assert not bits_equal(second[0], first[0])
    net.seed_dropout(12)
    other = small.step()
    assert not bits_equal(other[0], first[0])
    net.seed_dropout(11, calls=1)                                                     # and call 1 can be entered directly
    assert same(small.step(), second)


def test_layers_draw_different_masks(small):
    """6d. the masks of layers 0 and 1 in the same call (offsets calls * 1024 + layer) differ, and so do those of one layer in calls 0 and 1"""
    from viai_amd.wavenet import dropout_mask
    shape = (small.B, 1, small.T, small.cfg.residual_channels)
    m = {off: dropout_mask(shape, P, 11, off) for off in (0, 1, 1024)}
    assert not torch.equal(m[0], m[1]) and not torch.equal(m[0], m[1024]) and not torch.equal(m[1], m[1024])
    for v in m.values():                                                              # each near 1 - p: 8192 elements, sigma = 20
        assert abs(int(v.sum()) - 0.95 * v.numel()) < 120


def test_network_resumes_from_saved_state(small):
    """6e. dropout_state() taken after one step and loaded again reproduces the second step bit for bit"""
    net = small.net
    net.seed_dropout(11)
    small.step()
    saved = net.dropout_state()
    assert saved == {"seed": 11, "calls": [1] * small.cfg.layers}
    second = small.step()
    assert net.dropout_state()["calls"] == [2] * small.cfg.layers
    net.load_dropout_state(saved)
    assert same(small.step(), second)


def test_unseeded_network_follows_torch_manual_seed(small):
    """6e'. never seeded: the layers draw their seeds from torch's default CPU generator, so torch.manual_seed fixes the run"""
    runs = []
    for _ in range(2):
        small.net.load_dropout_state({"seed": None, "calls": [0] * small.cfg.layers})
        torch.manual_seed(1234)
        runs.append(small.step())
        assert all(isinstance(f._drop_seed, int) for f in small.net.conv_layers)
    assert same(runs[0], runs[1])


def test_eval_mode_is_the_network_without_dropout(small):
    """6f. .eval() logits equal those of the same weights built with dropout = 0.0, bit for bit, and no call is counted"""
    plain = build(small.cfg, 0.0).eval()
    small.net.seed_dropout(11)
    small.net.eval()
    try:
        with torch.no_grad():
            a = small.net.forward_nhwc(small.x, small.c)
            b = plain.forward_nhwc(small.x, small.c)
    finally:
        small.net.train()
    assert bits_equal(a, b) and small.net.dropout_state()["calls"] == [0] * small.cfg.layers


def test_dropout_zero_launches_nothing(small):
    """6g. with dropout = 0.0 in train mode viai_dropout is never launched (every dropout = 0 path keeps its bits); with 0.05 it runs once
    per layer and direction"""
    from viai_amd import _lib
    lib = _lib.load()
    real, calls = lib.viai_dropout, []

    def counting(*a):
        calls.append(a[2])
        return real(*a)
    plain = Net(dropout=0.0)
    lib.viai_dropout = counting
    try:
        plain.step()
        n_plain = len(calls)
        small.net.seed_dropout(11)
        small.step()
        n_drop = len(calls) - n_plain
    finally:
        lib.viai_dropout = real
    assert n_plain == 0
    assert n_drop == 2 * small.cfg.layers and set(calls) == {small.B * small.T * small.cfg.residual_channels}
    assert plain.net.dropout_state() == {"seed": None, "calls": [0] * small.cfg.layers}


# ----------------------------------------------------------------------------- 7. the one-hot network
def test_one_hot_network_trains_with_dropout():
    """7. forward_nhwc(classes) in train mode with dropout = 0.05 and the fused masked cross-entropy (shift = 1): finite loss and gradients,
    the same bits under the same seed, other bits under another"""
    from viai_amd.wavenet import masked_cross_entropy, sequence_mask
    cfg = W.WNConfigOneHot
    B, T, K = 2, 64, cfg.out_channels
    net = build(cfg, P, scalar_input=False)
    idx = (O.cf_uniform("drop.oh.idx", (B, T), 0, 1) * K).long().clamp(max=K - 1).cuda()
    c = O.cf_uniform("drop.oh.c", (B, cfg.cin_channels, T // 16), 0, 1).cuda()
    mask = sequence_mask(torch.tensor([T - 1, T - 15]).cuda(), T - 1)

    def step(seed):
        net.seed_dropout(seed)
        net.zero_grad(set_to_none=True)
        loss = masked_cross_entropy(net.forward_nhwc(idx, c), idx, mask, shift=1)
        loss.backward()
        return loss.detach().reshape(1), grads(net)
    a, b, other = step(11), step(11), step(12)
    assert torch.isfinite(a[0]).item() and all(torch.isfinite(v).all().item() for v in a[1].values())
    assert same(a, b) and not bits_equal(a[0], other[0])
