"""GPU: `janssen_fill` (csrc/janssen_fill.hip) against its host mirror BIT FOR BIT over the case table of tests/janssen_common.py, with the lists
read in place as device tensors and handed over as host arrays; a row alone against the row in a batch; and the pass-throughs `declick(...,
method="janssen")` and `repair(..., ar_method="janssen")` against the host composition.  The mirror itself is pinned to the numpy restatement
by tests/test_janssen_cpu.py."""
import numpy as np
import pytest
import torch

import ar_fill_common as A
import janssen_common as J

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


_HOST = {}


def host(c):
    from viai_amd.janssen import janssen_fill_host
    if c["name"] not in _HOST:
        _HOST[c["name"]] = janssen_fill_host(c["wav"][:, :c["n"]], c["gaps"], lengths=c["lengths"], **c["kw"])
    return _HOST[c["name"]]


@pytest.mark.parametrize("name", J.case_names())
def test_device_equals_the_host_mirror_bit_for_bit(name):
    from viai_amd.janssen import janssen_fill
    c = J.case_by_name(name)
    want, want_filled = host(c)
    wav = torch.from_numpy(np.ascontiguousarray(c["wav"][:, :c["n"]])).cuda()
    dev_gaps = tuple(torch.from_numpy(np.ascontiguousarray(g, dtype=np.int32)).cuda() for g in c["gaps"])
    before = wav.clone()
    out, filled = janssen_fill(wav, dev_gaps, lengths=c["lengths"], **c["kw"])          # the lists are read where they lie
    assert out.dtype == torch.float32 and filled.dtype == torch.int32 and out.is_cuda and filled.is_cuda
    assert np.array_equal(filled.cpu().numpy(), want_filled), (filled.cpu().numpy(), want_filled)
    assert np.array_equal(bits(out.cpu().numpy()), bits(want))
    assert torch.equal(wav.view(torch.int32), before.view(torch.int32))                  # the input is not written
    out2, filled2 = janssen_fill(wav, c["gaps"], lengths=None if c["lengths"] is None else c["lengths"].tolist(), **c["kw"])   # host lists
    assert torch.equal(out2.view(torch.int32), out.view(torch.int32)) and torch.equal(filled2, filled)


def test_a_row_alone_is_the_row_in_a_batch_of_four_and_twice_is_the_same():
    from viai_amd.janssen import janssen_fill
    for name in ("ragged rows", "lists that are not lists", "single gaps"):
        c = J.case_by_name(name)
        assert c["wav"].shape[0] == 4
        wav = torch.from_numpy(np.ascontiguousarray(c["wav"][:, :c["n"]])).cuda()
        g = tuple(torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).cuda() for x in c["gaps"])
        ln = None if c["lengths"] is None else torch.from_numpy(c["lengths"]).cuda()
        whole, filled = janssen_fill(wav, g, lengths=ln, **c["kw"])
        again, filled2 = janssen_fill(wav, g, lengths=ln, **c["kw"])
        assert torch.equal(whole.view(torch.int32), again.view(torch.int32)) and torch.equal(filled, filled2)
        for b in range(4):
            alone, f1 = janssen_fill(wav[b:b + 1], tuple(x[b:b + 1] for x in g), lengths=None if ln is None else ln[b:b + 1], **c["kw"])
            assert torch.equal(alone[0].view(torch.int32), whole[b].view(torch.int32)) and torch.equal(f1[0], filled[b]), (name, b)


def crackled():
    clean = J.crackle_clean()[:1].copy()
    hurt = clean.copy()
    pos = np.arange(1500, 1500 + 48 * 20, 48)
    hurt[0, pos] += np.where(np.arange(20) % 2 == 0, 0.5, -0.5).astype(np.float32)
    return hurt


def test_declick_janssen_equals_declick_host_with_the_lists_on_the_device():
    from viai_amd.click_detect import declick, declick_host
    hurt = crackled()
    want, want_gaps, want_filled = declick_host(hurt, method="janssen", ar_iters=2)
    assert 20 <= int(want_gaps.count[0]) <= 64
    out, gaps, filled = declick(torch.from_numpy(hurt).cuda(), method="janssen", ar_iters=2)
    assert all(t.is_cuda for t in gaps) and filled.is_cuda
    assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(gaps, want_gaps))
    assert np.array_equal(filled.cpu().numpy(), want_filled) and np.array_equal(bits(out.cpu().numpy()), bits(want))
    # the default is today's path
    from viai_amd.ar_fill import ar_fill
    out_b, gaps_b, filled_b = declick(torch.from_numpy(hurt).cuda())
    ref, ref_filled = ar_fill(torch.from_numpy(hurt).cuda(), gaps_b, order=32, context=1024)
    assert torch.equal(out_b.view(torch.int32), ref.view(torch.int32)) and torch.equal(filled_b, ref_filled)


def test_repair_with_ar_method_janssen_equals_the_host_composition():
    from viai_amd.ar_fill import ar_fill_host
    from viai_amd.gap_detect import repair
    from viai_amd.janssen import janssen_fill_host, rule_max_len
    rows = [J.CRACKLE_ROWS[2][:12], [(900, 40), (1000, 7)]]
    hurt = A.damage(J.crackle_clean()[:2], rows)
    gaps = A.lists(rows, 12)
    tg = tuple(torch.from_numpy(g).cuda() for g in gaps)
    out, _ = repair(None, torch.from_numpy(hurt).cuda(), gaps=tg, ar_below=64, ar_method="janssen", ar_iters=2)
    want, filled = janssen_fill_host(hurt, gaps, order=32, context=1024, iters=2, max_len=min(63, rule_max_len(32, 1024)))
    assert (filled[0] == 1).all() and filled[1].tolist() == [1, 1] + [0] * 10
    assert np.array_equal(bits(out.cpu().numpy()), bits(want))
    # the default is today's path
    out_b, _ = repair(None, torch.from_numpy(hurt).cuda(), gaps=tg, ar_below=64)
    assert np.array_equal(bits(out_b.cpu().numpy()), bits(ar_fill_host(hurt, gaps, order=32, context=1024, max_len=63)[0]))
    with pytest.raises(ValueError):                                                          # a run Janssen skips goes on to the inpainter
        repair(None, torch.from_numpy(hurt).cuda(), gaps=tg, ar_below=40, ar_method="janssen")
