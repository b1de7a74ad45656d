"""GPU: the ragged STFT -> mel call (MelFrontEnd.ragged, viai_stft_mel_ragged) against the one-clip call, row by row and BIT FOR BIT.

The contract (include/viai_hip.h): row r of a ragged call has the bits of a one-clip call on that row's samples, on the kernel family
viai_stft_mel_route names for the row's length and the alignment of its first sample.  A fresh copy of a row is 8-byte aligned, so "equals the
front end on a fresh copy" holds for rows whose first sample is 8-byte aligned and for odd-length rows anywhere (they run on the wave kernel either
way); an even-length row one float off alignment runs on the wave kernel and is compared with the one-clip call on an equally misaligned view.
The rows are packed back to back with loud samples up to both ends of every row: a neighbour read into a row's zero padding changes the bits of
its first and last frames.  The accuracy anchor (fp64 oracle) does not go through the one-clip call."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_preprocess_gpu import CHUNK, HOP, bits_equal, loud, trimmed_file
from test_stft_mel_routes_gpu import EPS32, MARGIN, pipe32, ref64

pytestmark = pytest.mark.gpu

# even-length rows at even offsets, odd-length rows at even AND odd offsets, no gap anywhere
LENS = [256, 1024, 1, 8191, 8192, 255, 8193, 8448, 257]
OFFS = [0, 256, 1280, 1281, 9472, 17664, 17919, 26112, 34560]
_fronts = {}


def front(hop=256):
    from viai_amd.audio import AudioConfig, MelFrontEnd
    if hop not in _fronts:
        class Cfg(AudioConfig):
            hop_size = hop
        _fronts[hop] = MelFrontEnd(AudioConfig if hop == 256 else Cfg, device="cuda")
    return _fronts[hop]


def packed(lens, seed):
    offs = [0] + np.cumsum(lens).tolist()[:-1]
    wav = loud(sum(lens), torch.Generator().manual_seed(seed)).cuda()
    assert wav.data_ptr() % 8 == 0 and float(wav.abs().min()) >= 0.1
    return wav, offs


def one_clip(f, wav, o, n, mask=None):
    """the front end on a FRESH copy of the row"""
    row = wav[o:o + n].clone()
    assert row.data_ptr() % 8 == 0
    return f(row[None], None if mask is None else mask[None])[0, 0]


def route_of(n, hop, aligned):
    from viai_amd import _lib
    buf = C.create_string_buffer(16)
    assert _lib.load().viai_stft_mel_route(n, 1024, hop, 80, int(aligned), buf, 16) == 1
    return buf.value.decode()


def assert_rows(got, want, time_major=False):
    assert len(got) == len(want)
    base = got[0].untyped_storage().data_ptr()
    for r, (g, w) in enumerate(zip(got, want)):
        assert g.is_contiguous() and g.untyped_storage().data_ptr() == base, r            # views of one allocation
        assert bits_equal(g, w.t() if time_major else w), "row %d (%s)" % (r, tuple(g.shape))


@pytest.fixture(scope="module")
def default_case():
    wav, offs = packed(LENS, 21)
    assert offs == OFFS
    f = front()
    want = [one_clip(f, wav, o, n) for o, n in zip(OFFS, LENS)]
    return wav, want


def test_rows_equal_the_one_clip_call(default_case):
    wav, want = default_case
    fams = [(n % 2, o % 2, route_of(n, 256, o % 2 == 0)) for n, o in zip(LENS, OFFS)]
    assert {(p, q) for p, q, _ in fams} == {(0, 0), (1, 0), (1, 1)} and {fam for _, _, fam in fams} == {"r512", "wave"}
    assert all(route_of(n, 256, o % 2 == 0) == route_of(n, 256, True) for n, o in zip(LENS, OFFS))      # the family of a fresh copy
    f = front()
    assert_rows(f.ragged(wav, LENS), want)
    assert_rows(f.ragged(wav, LENS, OFFS, time_major=True), want, time_major=True)
    # the same rows as a list of tensors (packed by the method at multiples of 4 samples) and, reversed, at explicit offsets
    assert_rows(f.ragged([wav[o:o + n] for o, n in zip(OFFS, LENS)]), want)
    assert_rows(f.ragged(wav, LENS[::-1], OFFS[::-1], time_major=True), want[::-1], time_major=True)


def test_even_rows_off_alignment_run_on_the_wave_kernel():
    """an even-length row whose first sample is one float off an 8-byte boundary: the wave family, the bits of a one-clip call on such a view"""
    lens = [1, 1024, 8192]
    wav, offs = packed(lens, 22)
    f = front()
    got = f.ragged(wav, lens)
    for r in (1, 2):
        assert offs[r] % 2 == 1 and route_of(lens[r], 256, False) == "wave" and route_of(lens[r], 256, True) == "r512"
        view = torch.zeros(lens[r] + 1, device="cuda")[1:]
        view.copy_(wav[offs[r]:offs[r] + lens[r]])
        assert view.data_ptr() % 8 == 4
        assert bits_equal(got[r], f(view[None])[0, 0]), r
    assert bits_equal(got[0], one_clip(f, wav, 0, 1))


@pytest.mark.parametrize("hop,family", [(200, None), (255, "banded")])
def test_other_hops(hop, family):
    lens = [256, 1024, 8191, 257]
    wav, offs = packed(lens, 23 + hop)
    assert [o % 2 for o in offs] == [0, 0, 0, 1]
    fams = {route_of(n, hop, o % 2 == 0) for n, o in zip(lens, offs)}
    assert fams == ({family} if family else {"r512", "wave"})
    f = front(hop)
    want = [one_clip(f, wav, o, n) for o, n in zip(offs, lens)]
    assert_rows(f.ragged(wav, lens), want)
    assert_rows(f.ragged(wav, lens, time_major=True), want, time_major=True)


@pytest.mark.parametrize("parity", [0, 1])
def test_persistent_loop(parity):
    """300 short rows and one of 70 000 samples in ONE family (even lengths: r512, odd: wave): 309 items on at most 256 blocks, so blocks take two
    items, a block's range crosses rows and the long row spans nine tiles"""
    from viai_amd.audio import lws_num_frames
    lens = [512 + 2 * ((37 * i) % 257) + parity for i in range(300)]
    lens.insert(150, 70000 + parity)
    assert min(lens) >= 512 and max(lens[:150] + lens[151:]) <= 1024 + parity and len(set(lens)) > 100
    items = sum(-(-lws_num_frames(n, 1024, 256) // 32) for n in lens)
    assert items == 309 > 256
    gen = torch.Generator().manual_seed(31 + parity)
    rows = [loud(n, gen).cuda() for n in lens]
    assert {route_of(n, 256, True) for n in lens} == {"wave" if parity else "r512"}
    f = front()
    want = [f(r.clone()[None])[0, 0] for r in rows]
    got = f.ragged(rows, time_major=bool(parity))
    assert_rows(got, want, time_major=bool(parity))


def test_mask_is_the_one_clip_calls(default_case):
    from viai_amd.audio import lws_num_frames
    wav, _ = default_case
    f = front()
    frames = [lws_num_frames(n, 1024, 256) for n in LENS]
    fo = [0] + np.cumsum(frames).tolist()
    mask = (torch.rand(fo[-1], generator=torch.Generator().manual_seed(41)) > 0.3).float()
    for r in range(len(LENS)):
        mask[fo[r]] = 0.0
        mask[fo[r + 1] - 1] = 0.0
    assert 0.3 < float(mask.mean()) < 0.9
    mask = mask.cuda()
    want = [one_clip(f, wav, o, n, mask[fo[r]:fo[r + 1]]) for r, (o, n) in enumerate(zip(OFFS, LENS))]
    assert all(float(w[:, 0].abs().max()) == 0.0 and float(w[:, -1].abs().max()) == 0.0 for w in want)
    assert all(float(w.abs().max()) > 0.0 for w, n in zip(want, LENS) if n >= 1024)          # ... and the rest of a row is not masked away
    assert_rows(f.ragged(wav, LENS, mask=mask), want)
    assert_rows(f.ragged(wav, LENS, mask=mask, time_major=True), want, time_major=True)


@pytest.mark.parametrize("hop", [256, 255])
@pytest.mark.parametrize("time_major", [0, 1])
def test_stores_stay_inside_the_output(default_case, time_major, hop):
    """the C entry on an output with sentinels in front of and behind the n_mels * total frames it may write (hop 255: the banded kernel)"""
    from viai_amd import _lib
    from viai_amd.audio import lws_num_frames
    lib = _lib.load()
    wav, _ = default_case
    f = front(hop)
    nr, G, SENT = len(LENS), 1021, 0x7FC12345
    off, ln = np.asarray(OFFS, np.int64), np.asarray(LENS, np.int32)
    frames, fo, per = np.zeros(nr, np.int32), np.zeros(nr + 1, np.int32), np.zeros(3, np.int32)
    args = (off.ctypes.data, ln.ctypes.data, nr, 1024, hop, 80, 1, frames.ctypes.data, fo.ctypes.data, None)
    need = lib.viai_stft_mel_ragged_plan(*args, None, 0, per.ctypes.data)
    items = np.zeros((need, 2), np.int32)
    assert need > 0 and lib.viai_stft_mel_ragged_plan(*args, items.ctypes.data, need, per.ctypes.data) == 0
    assert frames.tolist() == [lws_num_frames(n, 1024, hop) for n in LENS]
    total = int(fo[-1])
    d = [torch.from_numpy(a).cuda() for a in (off, ln, frames, fo, items)]
    buf = torch.full((2 * G + 80 * total,), SENT, dtype=torch.int32, device="cuda")
    out = buf[G:G + 80 * total]
    err = lib.viai_stft_mel_ragged(wav.data_ptr(), *[t.data_ptr() for t in d], per.ctypes.data, nr, f.window.data_ptr(), f.basis_t.data_ptr(),
                                   f.band_lo.data_ptr(), f.band_cnt.data_ptr(), 0, out.data_ptr(), 1024, hop, 80, time_major, -100.0, 20.0,
                                   torch.cuda.current_stream().cuda_stream)
    assert err == 0
    torch.cuda.synchronize()
    host = buf.cpu()
    assert bool((host[:G] == SENT).all()) and bool((host[G + 80 * total:] == SENT).all())
    assert not bool((host[G:G + 80 * total] == SENT).any())                                  # and every element inside was written
    got = f.ragged(wav, LENS, time_major=bool(time_major))
    assert torch.equal(torch.cat([g.reshape(-1) for g in got]).view(torch.int32).cpu(), host[G:G + 80 * total])


def test_accuracy_against_the_fp64_oracle(default_case):
    """the bound of tests/test_stft_mel_routes_gpu.py::norm_check, per row: min(2e-4, MARGIN x the fp32 restatement's worst error, floored at
    2 ulp of 1.0); the oracle and the restatement read the front end's own fp32 window and basis"""
    wav, _ = default_case
    f = front()
    win = f.window.cpu().numpy()
    basis = np.ascontiguousarray(f.basis_t.cpu().numpy().T)
    got = f.ragged(wav, LENS)
    host = wav.cpu().numpy()
    for r, (o, n) in enumerate(zip(OFFS, LENS)):
        row = host[None, o:o + n]
        ref = ref64(row, win, basis, 1024, 256, -100.0, 20.0)[0]
        cal = float(np.abs(pipe32(row, win, basis, 1024, 256, -100.0, 20.0).astype(np.float64) - ref).max())
        bound = min(2e-4, max(MARGIN * cal, 2.0 * EPS32))
        worst = float(np.abs(got[r].cpu().numpy()[None].astype(np.float64) - ref).max())
        print("row %d (%5d samples at %5d): fp32 restatement %.3e  bound %.3e  ragged worst %.3e  ratio %.2f" % (r, n, o, cal, bound, worst, worst / bound))
        assert worst <= bound, (r, worst, bound)


def test_preprocessor_takes_the_ragged_path():
    from viai_amd.preprocess import UtterancePreprocessor
    wav = trimmed_file(torch.Generator().manual_seed(51), lengths=(8 * HOP, 8 * HOP + 1, 9 * HOP - 1, 5 * HOP + 2)).cuda()
    f = front()
    recs = UtterancePreprocessor(front=f, chunk_samples=CHUNK, rescaling=False)(wav)
    assert len(recs) == 4
    assert len({r.mel.untyped_storage().data_ptr() for r in recs}) == 1                    # one allocation: the ragged call made them
    for r in recs:
        assert r.mel.is_contiguous() and r.mel.shape == (r.timesteps // HOP, 80) and r.mel.dtype == torch.float32
        assert bits_equal(r.mel, f(r.wav.clone()[None])[0, 0].t())

    class Plain:                                                                            # a user's front end: callable, no `ragged`
        cfg = f.cfg

        def __call__(self, wav, mask=None):
            return f(wav, mask)
    old = UtterancePreprocessor(front=Plain(), chunk_samples=CHUNK, rescaling=False)(wav)
    assert len({r.mel.untyped_storage().data_ptr() for r in old}) == 4
    for a, b in zip(recs, old):
        assert b.mel.is_contiguous() and bits_equal(a.mel, b.mel) and bits_equal(a.signal, b.signal) and (a.start, a.end, a.chunk) == (b.start, b.end, b.chunk)
