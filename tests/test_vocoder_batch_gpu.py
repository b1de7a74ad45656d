"""GPU: WaveNet training batches on the device (viai_amd.vocoder_batch, csrc/vocoder_batch.hip): every case of the reference's `collate_fn`
(tests/golden/vocoder_batch.npz), the kernel's shape edges and both of its access paths against a row-by-row torch composition, canaries round
every buffer, and a batch of `UtterancePreprocessor` pairs through the tiny one-hot WaveNet and the masked cross entropy.  Every expected value
is a copy, so every comparison but the last (class form against dense form, a different summation) is bit for bit."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CASES = ("no_crop", "crop", "exact_is_not_cropped", "one_window_short", "steps_not_divisible", "max_time_sec", "raw", "speaker_ids", "hop256")


def bits_equal(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return torch.equal(a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else torch.equal(a, b)


def batcher(**kw):
    from viai_amd.vocoder_batch import VocoderBatcher
    return VocoderBatcher(**kw)


def compose(rows, starts, frames, hop, K=None, T=None):
    """the batch row by row in torch: (y, classes, x, c) for int32 signals (x: the one-hot with zero columns for padding and for classes outside
    [0, K)), (y, None, x, c) with x = y's numbers for float signals"""
    B, L = len(rows), max(frames)
    T = L * hop if T is None else T
    L = T // hop
    dev = rows[0][0].device
    quant = rows[0][0].dtype == torch.int32
    sig = torch.zeros(B, T, dtype=rows[0][0].dtype, device=dev)
    c = None if rows[0][1] is None else torch.zeros(B, rows[0][1].shape[1], L, device=dev)
    for b, ((s, m), st, f) in enumerate(zip(rows, starts, frames)):
        sig[b, :f * hop] = s[st * hop:(st + f) * hop]
        if c is not None:
            c[b, :, :f] = m[st:st + f].t()
    if not quant:
        return sig.reshape(B, T, 1), None, sig.reshape(B, 1, T), c
    x = torch.zeros(B, K, T, device=dev)
    for b, f in enumerate(frames):
        k = sig[b, :f * hop].long()
        ok = (k >= 0) & (k < K)
        x[b, k[ok], torch.arange(f * hop, device=dev)[ok]] = 1.0
    return sig.long().reshape(B, T, 1), sig, x, c


def check(batch, want, what=""):
    y, classes, x, c = want
    assert bits_equal(batch.y, y), what
    if classes is None:
        assert batch.classes is None and bits_equal(batch.x, x) and batch.x.data_ptr() == batch.y.data_ptr(), what
    else:
        assert batch.classes.dtype == torch.int32 and torch.equal(batch.classes, classes), what
        if batch.x is not None:
            assert bits_equal(batch.x, x), what
    if c is None:
        assert batch.c is None, what
    else:
        assert bits_equal(batch.c, c), what


def random_rows(gen, n_frames, hop, D, K=256, dtype=torch.int32):
    rows = []
    for n in n_frames:
        sig = torch.randint(0, K, (n * hop,), generator=gen).int() if dtype == torch.int32 else torch.randn(n * hop, generator=gen)
        rows.append((sig.cuda(), None if D is None else torch.randn(n, D, generator=gen).cuda()))
    return rows


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "vocoder_batch.npz"))


@pytest.mark.parametrize("name", CASES)
def test_reference_fixture(golden, name):
    g = golden
    hop, D, mts, sr, K, seed = (int(v) for v in g[name + ".settings"])
    sec = float(g[name + ".max_time_sec"])
    kind = str(g[name + ".input_type"])
    n = g[name + ".n_frames"].tolist()
    sig, mel = torch.from_numpy(g[name + ".signal"]), torch.from_numpy(g[name + ".mel"])
    sig = sig.float() if kind == "raw" else sig.int()
    rows, a = [], 0
    for f in n:
        rows.append((sig[a * hop:(a + f) * hop].cuda(), mel[a:a + f].cuda()))
        a += f
    speakers = g[name + ".speakers"].tolist() if name + ".speakers" in g.files else None
    vb = batcher(hop=hop, input_type=kind, quantize_channels=K, max_time_steps=None if mts < 0 else mts, max_time_sec=None if np.isnan(sec) else sec,
                 sample_rate=sr, one_hot=kind != "raw")
    batch = vb(rows, rng=np.random.RandomState(seed), speaker_ids=speakers)
    y = torch.from_numpy(g[name + ".y"])
    lengths = torch.from_numpy(g[name + ".input_lengths"])
    assert batch.starts == g[name + ".starts"].tolist() and [f * hop for f in batch.frames] == lengths.tolist()
    assert batch.input_lengths.dtype == torch.int64 and batch.input_lengths.is_cuda and torch.equal(batch.input_lengths.cpu(), lengths)
    assert bits_equal(batch.c, torch.from_numpy(g[name + ".c"]))
    B, T = y.shape[0], y.shape[1]
    if kind == "raw":
        assert bits_equal(batch.y, y) and bits_equal(batch.x, y.reshape(B, 1, T)) and batch.classes is None
    else:
        y = y.long()
        assert batch.y.dtype == torch.int64 and torch.equal(batch.y.cpu(), y) and torch.equal(batch.classes.cpu(), y[:, :, 0].int())
        # the reference's x, as the fixture's tool asserted it: the one-hot of y with zero columns at t >= length
        x = torch.nn.functional.one_hot(y[:, :, 0], K).float() * (torch.arange(T)[None, :, None] < lengths[:, None, None])
        assert bits_equal(batch.x, x.transpose(1, 2))
    if speakers is None:
        assert batch.g is None
    else:
        assert batch.g.dtype == torch.int64 and torch.equal(batch.g.cpu(), torch.from_numpy(g[name + ".g"]))


# hop, D, K, frames, frames kept by the crop (None: no crop), injected starts, pad_to
EDGES = {
    "hop4": (4, 80, 256, (3, 5, 6, 9), 5, (0, 0, 1, 3), None),
    "hop4_small": (4, 3, 8, (3, 5, 6, 9), 5, (0, 0, 0, 4), None),
    "hop256_crosses_the_signal_tile": (256, 80, 256, (3, 5, 6, 9), 5, (0, 0, 1, 2), None),             # T = 1280 > 1024
    "hop256_small": (256, 3, 8, (3, 5, 6, 9), 5, (0, 0, 1, 4), None),
    "hop5_element_wise": (5, 80, 8, (3, 5, 6, 9), 5, (0, 0, 1, 3), None),                              # odd hop, T % 4 != 0
    "hop5_small": (5, 3, 256, (3, 5, 6, 9), 5, (0, 0, 0, 1), None),
    "frames_cross_the_transpose_tile": (4, 80, 256, (33, 40), None, (0, 0), None),                     # L = 40 > 32
    "one_row": (4, 80, 8, (7,), None, (0,), None),
    "pad_to": (4, 3, 8, (3, 5), None, (0, 0), 30),                                                     # T = 32, L = 8
    "pad_to_hop256": (256, 80, 256, (3, 5), None, (0, 0), 1281),                                       # T = 1536, L = 6
}


@pytest.mark.parametrize("name", sorted(EDGES))
def test_shape_edges(name):
    hop, D, K, n, keep, starts, pad_to = EDGES[name]
    gen = torch.Generator().manual_seed(sorted(EDGES).index(name))
    rows = random_rows(gen, n, hop, D, K)
    vb = batcher(hop=hop, quantize_channels=K, max_time_steps=None if keep is None else keep * hop, one_hot=True, pad_to=pad_to)
    batch = vb(rows, starts=list(starts))
    frames = [min(f, keep or f) for f in n]
    assert batch.starts == list(starts) and batch.frames == frames
    T = None if pad_to is None else -(-max(max(frames) * hop, pad_to) // hop) * hop
    check(batch, compose(rows, starts, frames, hop, K, T), name)
    assert batch.y.shape[1] == (T or max(frames) * hop) and torch.equal(batch.input_lengths.cpu(), torch.tensor(frames) * hop)
    # the class form alone (no x) writes the same y / classes / c
    lean = batcher(hop=hop, quantize_channels=K, max_time_steps=None if keep is None else keep * hop, pad_to=pad_to)(rows, starts=list(starts))
    assert lean.x is None and torch.equal(lean.y, batch.y) and torch.equal(lean.classes, batch.classes) and bits_equal(lean.c, batch.c)


@pytest.mark.parametrize("hop", [4, 256, 5])
def test_misaligned_sources_give_the_same_bits(hop):
    gen = torch.Generator().manual_seed(20 + hop)
    n, starts, D, K = (6, 9, 4), [1, 2, 0], 80, 256
    rows = random_rows(gen, n, hop, D, K)
    off = []
    for s, m in rows:                                                       # views that start one element into their buffers
        sb, mb = torch.empty(s.numel() + 1, dtype=s.dtype, device="cuda"), torch.empty(m.numel() + 1, device="cuda")
        sb[1:], mb[1:] = s, m.reshape(-1)
        off.append((sb[1:], mb[1:].view(m.shape)))
        assert off[-1][0].data_ptr() % 16 == 4 and off[-1][1].data_ptr() % 16 == 4
    vb = batcher(hop=hop, max_time_steps=5 * hop, one_hot=True)
    a, b = vb(rows, starts=starts), vb(off, starts=starts)
    for u, v in ((a.y, b.y), (a.classes, b.classes), (a.x, b.x), (a.c, b.c)):
        assert bits_equal(u, v)
    check(b, compose(rows, starts, [5, 5, 4], hop, K))


def test_a_class_out_of_range_is_a_zero_column():
    K, hop = 8, 4
    sig = torch.tensor([3, K, -1, 7, 0, K + 100, -2 ** 31, 2 ** 31 - 1], dtype=torch.int32).cuda()
    rows = [(sig, torch.ones(2, 3).cuda()), (sig.flip(0).contiguous(), torch.ones(2, 3).cuda())]
    batch = batcher(hop=hop, quantize_channels=K, one_hot=True)(rows)
    assert torch.equal(batch.y[:, :, 0], torch.stack([sig, sig.flip(0)]).long()) and torch.equal(batch.classes, torch.stack([sig, sig.flip(0)]))
    want = torch.zeros(2, K, 8)
    want[0, 3, 0] = want[0, 7, 3] = want[0, 0, 4] = 1.0
    want[1, :, :] = want[0].flip(1)
    assert bits_equal(batch.x, want)


@pytest.mark.parametrize("hop,mode", [(4, 0), (5, 0), (256, 0), (4, 2)])
def test_canaries_round_every_buffer(hop, mode):
    """the C entry point on over-allocated outputs full of a sentinel, the source rows each directly in front of a sentinel tail: nothing is written
    outside [B][T_out], [B][K][T_out], [B][D][L_out], and no sentinel is read into them (every padded position is 0, not the tail's value)"""
    from viai_amd import _lib
    lib = _lib.load()
    gen = torch.Generator().manual_seed(40 + hop)
    n, keep, D, K, PAD = (7, 3, 6), 5, 80, 8, 1024
    starts, frames = [2, 0, 1], [5, 3, 5]                                    # rows 0 and 2: the window ends where the row ends
    L = 6                                                                    # one frame of padding for every row
    T = L * hop
    dtype = torch.int32 if mode == 0 else torch.float32
    sent_sig = 5 if mode == 0 else 777.0                                     # a valid class: it would light up x
    rows = random_rows(gen, n, hop, D, K, dtype)
    src = []
    for s, m in rows:
        sb = torch.full((s.numel() + PAD,), sent_sig, dtype=dtype, device="cuda")
        mb = torch.full((m.numel() + PAD,), 1e30, device="cuda")
        sb[:s.numel()], mb[:m.numel()] = s, m.reshape(-1)
        src.append((sb, mb))
    tab = torch.tensor([sb.data_ptr() for sb, _ in src] + [mb.data_ptr() for _, mb in src], dtype=torch.int64).cuda()
    plan = torch.tensor(starts + frames, dtype=torch.int32).cuda()
    B = len(rows)
    y = torch.full((B * T + PAD,), -7, dtype=torch.int64 if mode == 0 else torch.float32, device="cuda")
    classes = torch.full((B * T + PAD,), -7, dtype=torch.int32, device="cuda")
    x = torch.full((B * K * T + PAD,), -7.0, device="cuda")
    c = torch.full((B * D * L + PAD,), -7.0, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.viai_voc_collate(tab.data_ptr(), tab.data_ptr() + 8 * B, plan.data_ptr(), plan.data_ptr() + 4 * B, B, hop, D, mode, K, T, L, y.data_ptr(),
                                    classes.data_ptr() if mode == 0 else 0, x.data_ptr() if mode == 0 else 0, c.data_ptr(), st), "viai_voc_collate")
    want_y, want_cls, want_x, want_c = compose(rows, starts, frames, hop, K, T)
    assert bits_equal(y[:B * T], want_y.reshape(-1)) and bool((y[B * T:] == -7).all())
    assert bits_equal(c[:B * D * L].view(B, D, L), want_c) and bool((c[B * D * L:] == -7.0).all())
    if mode == 0:
        assert torch.equal(classes[:B * T].view(B, T), want_cls) and bool((classes[B * T:] == -7).all())
        assert bits_equal(x[:B * K * T].view(B, K, T), want_x) and bool((x[B * K * T:] == -7.0).all())
    else:
        assert bool((classes == -7).all()) and bool((x == -7.0).all())      # not touched in the float modes
    for b, f in enumerate(frames):                                           # the padding is zero: the tails were not read
        assert not bool(y[b * T + f * hop:(b + 1) * T].any()) and not bool(c[:B * D * L].view(B, D, L)[b, :, f:].any())


@pytest.mark.parametrize("kind", ["raw", "mulaw"])
def test_float_modes_carry_the_source_bits(kind):
    gen = torch.Generator().manual_seed(50)
    hop, n, starts = 4, (6, 9, 3), [1, 3, 0]
    rows = random_rows(gen, n, hop, 6, dtype=torch.float32)
    rows[0][0][4:8] = torch.tensor([-0.0, float("inf"), 1e-42, -1.0]).cuda()                 # signs, an infinity and a denormal travel as bits
    batch = batcher(hop=hop, input_type=kind, max_time_steps=5 * hop)(rows, starts=starts)
    assert batch.x.shape == (3, 1, 20) and batch.y.shape == (3, 20, 1) and batch.x.dtype == batch.y.dtype == torch.float32
    check(batch, compose(rows, starts, [5, 5, 3], hop))
    assert bits_equal(batch.x[2, 0, 12:], torch.zeros(8)) and bits_equal(batch.y[2, 12:, 0], torch.zeros(8))      # +0.0, bit for bit
    plain = batcher(hop=hop, input_type=kind)([(s, None) for s, _ in rows])                     # no mel, no crop
    assert plain.c is None and plain.x.shape == (3, 1, 36) and bits_equal(plain.x[1, 0], rows[1][0])


def test_two_calls_give_the_same_bits():
    gen = torch.Generator().manual_seed(60)
    rows = random_rows(gen, (6, 9, 12), 256, 80)
    vb = batcher(max_time_steps=5 * 256 + 100, one_hot=True)
    a, b = vb(rows, rng=np.random.RandomState(3)), vb(rows, rng=np.random.RandomState(3))
    assert a.starts == b.starts and a.frames == b.frames == [5, 5, 5]
    for u, v in ((a.y, b.y), (a.classes, b.classes), (a.x, b.x), (a.c, b.c), (a.input_lengths, b.input_lengths)):
        assert bits_equal(u, v)


def test_argument_checks_on_device_tensors():
    gen = torch.Generator().manual_seed(70)
    (sig, mel), = random_rows(gen, (4,), 4, 6)
    vb = batcher(hop=4)
    for bad in ([(sig.float(), mel)], [(sig, mel.double())]):
        with pytest.raises(TypeError):
            vb(bad)
    for bad in ([(sig[:15], mel)], [(sig[:12], mel)], [(sig, mel[:3])], [(sig, mel.t().contiguous().t())], [(sig.repeat(2)[::2], mel)],
                [(sig, mel), (sig, mel[:, :5].contiguous())], [(sig, mel), (sig, None)], [(sig.reshape(4, 4), mel)]):
        with pytest.raises(ValueError):
            vb(bad)
    with pytest.raises(ValueError):
        vb([(sig, mel)], speaker_ids=[1, 2])
    with pytest.raises(ValueError):
        batcher(hop=4, max_time_steps=8)([(sig, mel)], starts=[3])          # 0 <= s <= n - L = 2


FFT, HOP, MELS, CHUNK = 1024, 256, 80, 4096
# the tolerance tests/test_wavenet_onehot_train_gpu.py applies where it compares the class form with the dense form of the same network (1e-4 relative,
# its test 8; the same bound it puts on the loss against the reference in its test 5): the two forms sum the first conv in different orders
CLASS_VS_DENSE = 1e-4


def loud(n, gen, lo=0.1, hi=0.9):
    mag = lo + (hi - lo) * torch.rand(n, generator=gen)
    return mag * (torch.randint(0, 2, (n,), generator=gen) * 2 - 1).float()


def test_a_batch_trains_a_tiny_one_hot_wavenet():
    """three pairs from `UtterancePreprocessor` as tests/test_preprocess_gpu.py builds them (one chunk each: silence, loud samples, silence), the
    middle one 4 frames short so that it is padded; cropped to 5 frames; the pair test's tiny network and the fused masked cross entropy"""
    from viai_amd.audio import AudioConfig, MelFrontEnd
    from viai_amd.preprocess import UtterancePreprocessor
    from viai_amd.wavenet import MaskedCrossEntropyLoss, WaveNet
    gen = torch.Generator().manual_seed(11)
    parts = []
    for T in (8 * HOP, 100, 9 * HOP - 1):
        chunk = torch.zeros(CHUNK)
        chunk[100:100 + T + 1] = loud(T + 1, gen)
        parts.append(chunk)
    recs = UtterancePreprocessor(front=MelFrontEnd(AudioConfig, device="cuda"), chunk_samples=CHUNK, rescaling=False)(torch.cat(parts).cuda())
    assert [r.mel.shape[0] for r in recs] == [11, 4, 12]
    kw = dict(max_time_steps=5 * HOP + 100)
    batch = batcher(one_hot=True, **kw)(recs, rng=np.random.RandomState(0))
    assert batch.frames == [5, 4, 5] and batch.starts[1] == 0 and batch.classes.shape == (3, 5 * HOP) and batch.c.shape == (3, MELS, 5)
    lean = batcher(**kw)(recs, starts=batch.starts)
    assert lean.x is None and torch.equal(lean.classes, batch.classes) and bits_equal(lean.c, batch.c)
    torch.manual_seed(0)
    net = WaveNet(out_channels=256, layers=4, stacks=2, residual_channels=16, gate_channels=16, skip_out_channels=16, dropout=0.0, cin_channels=MELS,
                  upsample_scales=[4, 4, 4, 4], scalar_input=False).cuda()
    crit = MaskedCrossEntropyLoss()
    T = 5 * HOP

    def loss_of(x, c, y, lengths):
        with torch.no_grad():
            return crit(net.forward_nhwc(x, c), y, lengths=lengths, max_len=T - 1, shift=1)
    loss = loss_of(lean.classes, lean.c, lean.y, lean.input_lengths)
    assert torch.isfinite(loss).item() and loss.item() > 0
    # the same batch assembled row by row in torch from the same pairs and starts
    y, classes, x, c = compose([(r.signal, r.mel) for r in recs], batch.starts, batch.frames, HOP, 256)
    lengths = torch.tensor([f * HOP for f in batch.frames]).cuda()
    assert bits_equal(loss, loss_of(classes, c, y, lengths))
    dense = loss_of(batch.x, batch.c, batch.y, batch.input_lengths)
    print("loss: class form %.9g, dense form %.9g" % (loss.item(), dense.item()))
    assert abs(dense.item() - loss.item()) < CLASS_VS_DENSE * loss.item()
