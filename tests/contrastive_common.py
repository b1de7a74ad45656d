"""Shared helpers of the direct tests of csrc/contrastive.hip and of viai_l2_ranks in csrc/pipeline.hip (test_contrastive_inputs_cpu.py,
test_contrastive_pipeline_passes_gpu.py).  No GPU and no library here: fp64 truths, their fp32 restatements (the scale of
passes_common.bound_abs / check_abs / check_rel), the input builders with their planted ties, and the decision margins.

THE CONTRASTIVE LOSS.  scores[a][b] = ||f1[a] - f2[b]||, the loss as oracle/viai_oracle.py::l2_contrastive, the gradients in closed form (no autograd):

    df1[a] = g * sum_b w_ab (f1[a] - f2[b])          df2[b] = -g * sum_a w_ab (f1[a] - f2[b])
    w_aa = 1/n;   off the diagonal w_ab = -(margin - s_ab) / (n * s_ab) where the hinge is active (margin - s_ab > 0) and, under max_violation,
    b is the FIRST maximum of the row's hinge costs;   w_ab = 0 where s_ab = 0 (torch itself returns NaN there).

The fp64 truth evaluates the two sums factorised (rowsum(W) * f1 - W @ f2): in fp64 the cancellation that costs is 1e-16 of the operands, nothing
against an fp32 bound.  The fp32 restatement sums w_ab * (f1[a] - f2[b]) pair by pair, as the kernel does.  closed_form_vs_autograd() pins the
closed form against fp64 autograd of the oracle wherever no distance is zero.

PLANTED TIES (n >= 5, l2c_plan): f2[p] == f2[q] bit for bit and close to f1[a0], so that row a0 has two equal, largest hinge costs (the first one
must win the arg-max); f1[far] is three times a draw, so that its row lies beyond every other distance (a row with no active hinge);
f2[z] == f1[z] (distance exactly 0 on the diagonal) and f2[y] == f1[x] (exactly 0 off it).

RETRIEVAL (ret_inputs).  Two input families.  "c": clips uniform, captions = clips + half-amplitude noise.  "g": every coordinate a multiple of
1/8 in [-1, 1], so that every squared distance is a multiple of 1/64, at most 4 * dim <= 2^15, and EXACT in fp32 in any summation order, with or without fma:
rounding cannot flip a decision, every natural tie is a true tie in fp64 too and is decided by index (the oracle sorts stably), and the ranks
spread over the whole range.  Planted in both (n_clips >= 5, ret_plan): clips[jl] == clips[i0] == clips[jh] with jl < i0 < jh (a tie with the
matching clip below and above it) and clips[k1] == clips[k2] nearest to caption i1 (a tie for top-1).

THE CONDITION.  Hinge, arg-max and rank decisions are discrete; fp32 may flip one that sits on a rounding boundary, and that is no kernel error.
Every case used on the GPU therefore meets: each decision margin (decision_margins / ret_decision_margins, from the fp64 truth alone) exceeds
COND x the fp32 restatement's worst error on the quantity compared (the score; for retrieval the squared distance), measured at that shape.  For
the "g" family that error is exactly 0 and so is the margin required.  tests/test_contrastive_inputs_cpu.py asserts it for every case."""
import functools

import numpy as np
import torch

from oracle import viai_oracle as O
from passes_common import uniform

COND = 64.0

# (n, d): every n of {1, 2, 5, 6, 64, 257, 300} (n % 4 in {0, 1, 2, 3}; one row / two rows per thread of the loss; one / two arg-max blocks) and
# every d of {1, 63, 64, 65, 256, 300} (d < 64, = 64, % 64 != 0, > 256)
L2C_SHAPES = [(1, 1), (1, 64), (2, 63), (2, 300), (5, 65), (5, 256), (6, 1), (6, 64), (6, 300), (64, 63), (64, 256), (257, 64), (257, 65),
              (300, 256), (300, 300)]
MARGIN_KINDS = ("zero", "row", "mid", "all")
# the draw of each shape, where seed 0 misses THE CONDITION at some margin kind or meets it by a hair: the first seed that leaves a quarter of room
# (at n = 300 about one seed in two meets it at all: 90 000 distances lie within +-1 of each other, and fp32 resolves them to 3e-6)
L2C_SEEDS = {(257, 65): 1, (300, 300): 11}

# (n_clips, n_captions, dim, family)
RET_CASES = [(1, 1, 1, "c"), (1, 1, 64, "g"), (5, 5, 1, "c"), (5, 3, 64, "c"), (5, 5, 8192, "c"), (5, 3, 8192, "g"), (255, 255, 64, "c"),
             (255, 100, 64, "g"), (256, 256, 64, "g"), (256, 200, 1, "g"), (257, 257, 64, "c"), (257, 200, 64, "g"), (700, 700, 64, "c"),
             (700, 300, 64, "g"), (700, 700, 1, "g")]
# likewise for retrieval
RET_SEEDS = {(257, 257, 64, "c"): 1}


def f32(x):
    """the fp32 value the C ABI receives for a Python float"""
    return float(np.float32(x))


# ---------------------------------------------------------------------------------------------------------------- contrastive: inputs

def l2c_plan(n):
    """rows of the planted ties, or None below n = 5"""
    if n < 5:
        return None
    return dict(a0=0, p=1, q=n - 2, z=2, x=n - 2, y=n - 1, far=1)


@functools.lru_cache(maxsize=None)
def _l2c_inputs(n, d, ties, zeros, seed):
    tag = "l2c.%d.%d.s%d" % (n, d, seed)
    f1 = uniform(tag + ".f1", (n, d)).clone()
    f2 = uniform(tag + ".f2", (n, d)).clone()
    pl = l2c_plan(n)
    if pl is not None:
        f1[pl["far"]] *= 3.0
        if ties:
            f2[pl["p"]] = f1[pl["a0"]] + 0.25 * uniform(tag + ".near", (d,))
            f2[pl["q"]] = f2[pl["p"]]
        if zeros:
            f2[pl["z"]] = f1[pl["z"]]
            f2[pl["y"]] = f1[pl["x"]]
    return f1, f2


def l2c_inputs(n, d, ties=True, zeros=True, seed=None):
    """f1, f2 (n, d) fp32 with the planted rows of l2c_plan(n); shared, do not write to them"""
    return _l2c_inputs(n, d, ties, zeros, L2C_SEEDS.get((n, d), 0) if seed is None else seed)


# ---------------------------------------------------------------------------------------------------------------- contrastive: truth

def scores_of(f1, f2, dtype):
    """fp64: the plain formula.  fp32: as l2c_scores_kernel states it -- 64 lanes, lane l adds the squares of coordinates l, l + 64, ... in turn,
    then the 64 partial sums are added by halving -- and with element-wise fp32 operations only, so that the restatement's error, and with it
    THE CONDITION, is the same on every machine (torch's own sum() changes its order with the CPU's vector width and thread count)"""
    a, b = f1.to(dtype), f2.to(dtype)
    if dtype == torch.float64:
        return (a[:, None, :] - b[None, :, :]).pow(2).sum(-1).sqrt()
    n, d = a.shape
    D = (d + 63) // 64 * 64
    a, b = torch.nn.functional.pad(a, (0, D - d)), torch.nn.functional.pad(b, (0, D - d))         # a padded lane adds exactly 0
    acc = torch.zeros(n, n, 64, dtype=dtype)
    for j in range(0, D, 64):
        t = a[:, None, j:j + 64] - b[None, :, j:j + 64]
        acc += t * t
    w = 64
    while w > 1:
        w //= 2
        acc = acc[..., :w] + acc[..., w:2 * w]
    return acc[..., 0].sqrt()


def argmax_rows(scores, margin):
    """the row's FIRST maximum of clamp(margin - s, 0) over b != a (the first b != a where nothing is violated); -1 at n = 1"""
    n = scores.shape[0]
    if n == 1:
        return np.full((1,), -1, dtype=np.int32)
    cost = (torch.tensor(margin, dtype=scores.dtype) - scores).clamp_min(0).numpy().copy()
    np.fill_diagonal(cost, -1.0)
    return np.argmax(cost, axis=1).astype(np.int32)                 # numpy documents the first occurrence


def weights(scores, margin, max_violation):
    """(W, arg, cost) in the dtype of scores: W as in the module docstring, cost the hinge costs with a zero diagonal"""
    n = scores.shape[0]
    dt = scores.dtype
    eye = torch.eye(n, dtype=torch.bool)
    cost = (torch.tensor(margin, dtype=dt) - scores).clamp_min(0).masked_fill(eye, 0)
    arg = argmax_rows(scores, margin)
    active = (cost > 0) & (scores > 0) & ~eye
    if max_violation:
        active &= torch.arange(n)[None, :] == torch.from_numpy(arg.astype(np.int64))[:, None]
    fn = torch.tensor(float(n), dtype=dt)
    W = torch.where(active, -cost / (fn * scores.clamp_min(1e-30)), torch.zeros((), dtype=dt))
    W = torch.where(eye & (scores > 0), torch.ones((), dtype=dt) / fn, W)
    return W, arg, cost


def loss_of(scores, cost, max_violation):
    n = scores.shape[0]
    hinge = (cost.max(1)[0] ** 2).sum() if max_violation else (cost ** 2).sum()
    return ((hinge + (scores.diag() ** 2).sum()) / (2 * n)).reshape(1)


def l2c_ref64(f1, f2, scores, margin, max_violation, g=1.0):
    """fp64 truth from the fp64 scores: dict(loss, arg, df1, df2, W)"""
    a, b = f1.double(), f2.double()
    W, arg, cost = weights(scores, margin, max_violation)
    df1 = g * (W.sum(1, keepdim=True) * a - W @ b)
    df2 = -g * (W.t() @ a - W.sum(0)[:, None] * b)
    return dict(loss=loss_of(scores, cost, max_violation), arg=arg, df1=df1, df2=df2, W=W)


def l2c_ref32(f1, f2, scores32, margin, max_violation, g=1.0):
    """the same formulas in fp32 with torch, pair by pair as the kernel sums them"""
    W, arg, cost = weights(scores32, margin, max_violation)
    diff = f1[:, None, :] - f2[None, :, :]
    g32 = torch.tensor(g, dtype=torch.float32)
    df1 = g32 * torch.einsum("ab,abk->ak", W, diff)
    df2 = -g32 * torch.einsum("ab,abk->bk", W, diff)
    return dict(loss=loss_of(scores32, cost, max_violation), arg=arg, df1=df1, df2=df2, W=W)


def closed_form_vs_autograd(f1, f2, margin, max_violation, merge=None):
    """worst |closed form - fp64 autograd of the oracle| over df1 and df2, relative to the largest gradient entry.  No distance may be zero.  Which
    of two exactly tied maxima torch's max() differentiates is its own affair: merge = (p, q) adds row q of df2 to row p on both sides first"""
    a = f1.double().clone().requires_grad_(True)
    b = f2.double().clone().requires_grad_(True)
    loss = O.l2_contrastive(a, b, margin, bool(max_violation))
    loss.backward()
    s = scores_of(f1, f2, torch.float64)
    assert float(s.min()) > 0.0
    ref = l2c_ref64(f1, f2, s, margin, max_violation)
    assert abs(float(ref["loss"]) - float(loss.detach())) <= 1e-13 * max(1.0, abs(float(loss.detach())))
    ga, gb, df2 = a.grad, b.grad.clone(), ref["df2"].clone()
    if merge is not None:
        p, q = merge
        gb[p] += gb[q]; gb[q] = 0
        df2[p] += df2[q]; df2[q] = 0
    scale = max(float(ga.abs().max()), float(gb.abs().max()), 1e-300)
    return max(float((ref["df1"] - ga).abs().max()), float((df2 - gb).abs().max())) / scale


# ---------------------------------------------------------------------------------------------------------------- contrastive: margins

def l2c_margin(scores, kind):
    """the margin of a kind, from the fp64 scores, as the fp32 value the C ABI receives.
      zero  0: no hinge is active anywhere, the loss is the diagonal term alone (the module's default)
      row   just below the largest of the rows' smallest off-diagonal distances (halfway down to the next distance of another row): that row -- the
            planted far row where there is one -- has no active hinge, every other row has
      mid   the middle of the widest gap of the sorted off-diagonal distances between their 5 % and 50 % quantiles: part active, part not
      all   1.25 x the largest distance: every hinge is active"""
    n = scores.shape[0]
    if kind == "zero":
        return 0.0
    if n == 1:
        return {"row": 0.5, "mid": 1.0, "all": 2.0}[kind]
    off = scores[~torch.eye(n, dtype=torch.bool)].reshape(n, n - 1)
    if kind == "all":
        return f32(1.25 * float(off.max()))
    if kind == "row":
        m, r = torch.sort(off.min(1)[0])
        below = torch.cat([off[:int(r[-1])], off[int(r[-1]) + 1:]]).reshape(-1)
        return f32(0.5 * (float(m[-1]) + float(below[below < m[-1]].max())))
    v = torch.unique(off.reshape(-1))                                # sorted
    v = v[v > 0]
    lo, hi = int(0.05 * (v.numel() - 1)), max(int(0.5 * (v.numel() - 1)), int(0.05 * (v.numel() - 1)) + 1)
    gaps = v[lo + 1:hi + 1] - v[lo:hi]
    k = lo + int(torch.argmax(gaps))
    return f32(0.5 * (float(v[k]) + float(v[k + 1])))


def decision_margins(scores, margin, plan, ties=True, zeros=True):
    """from the fp64 scores alone: (hinge, top2).
      hinge  the smallest |margin - s_ab| over the off-diagonal pairs whose distance is not a planted zero
      top2   the smallest gap between the two largest hinge costs of a row, over the rows that violate at all; where the two largest are the
             planted equal pair, the gap from the pair to the third"""
    n = scores.shape[0]
    if n == 1:
        return float("inf"), float("inf")
    mask = ~torch.eye(n, dtype=torch.bool)
    if plan is not None and zeros:
        mask[plan["x"], plan["y"]] = False
    hinge = float((margin - scores[mask]).abs().min())
    cost = (margin - scores).clamp_min(0).numpy().copy()
    np.fill_diagonal(cost, -np.inf)
    order = np.argsort(-cost, axis=1, kind="stable")
    top2 = float("inf")
    for a in range(n):
        c = cost[a, order[a]]
        if c[0] <= 0 or n < 3:
            continue
        k = 1
        if plan is not None and ties and {int(order[a, 0]), int(order[a, 1])} == {plan["p"], plan["q"]}:
            assert c[0] == c[1]
            k = 2
        if k < n - 1:
            top2 = min(top2, float(c[0] - c[k]))
    return hinge, top2


@functools.lru_cache(maxsize=4)
def l2c_scores(n, d, seed=None):
    """(f1, f2, scores64, scores32, error of scores32) of a shape: computed once, shared"""
    f1, f2 = l2c_inputs(n, d, seed=seed)
    s64, s32 = scores_of(f1, f2, torch.float64), scores_of(f1, f2, torch.float32)
    return f1, f2, s64, s32, float((s32.double() - s64).abs().max())


def l2c_condition(n, d, seed=None):
    """per margin kind and max_violation: (margin, worst fp32 error of a score, hinge margin, top-two margin or inf)"""
    f1, f2, s64, s32, err = l2c_scores(n, d, seed)
    out = {}
    for kind in MARGIN_KINDS:
        m = l2c_margin(s64, kind)
        hinge, top2 = decision_margins(s64, m, l2c_plan(n))
        out[kind] = (m, err, hinge, top2)
    return out


def l2c_condition_holds(n, d, seed=None):
    return all(h > COND * e and t > COND * e for (_, e, h, t) in l2c_condition(n, d, seed).values())


# ---------------------------------------------------------------------------------------------------------------- retrieval

def ret_plan(n_clips, n_cap):
    if n_clips < 5 or n_cap < 3:
        return None
    return dict(i0=2, jl=0, jh=n_clips - 1, k1=1, k2=3, i1=3 if n_cap >= 4 else 1)


def _grid(t):
    return torch.round(t * 8.0) / 8.0


@functools.lru_cache(maxsize=None)
def _ret_inputs(n_clips, n_cap, dim, family, seed):
    tag = "ret.%d.%d.%d.%s.s%d" % (n_clips, n_cap, dim, family, seed)
    clips = uniform(tag + ".clips", (n_clips, dim)).clone()
    noise = uniform(tag + ".noise", (n_cap, dim))
    near = uniform(tag + ".near", (dim,))
    if family == "g":
        clips = _grid(clips)
        caps = _grid(0.1 * clips[:n_cap] + 0.9 * noise)         # weakly tied to its clip: the ranks spread
    else:
        caps = clips[:n_cap] + 0.5 * noise
    pl = ret_plan(n_clips, n_cap)
    if pl is not None:
        clips[pl["jl"]] = clips[pl["i0"]]
        clips[pl["jh"]] = clips[pl["i0"]]
        if family == "g":
            clips[pl["k1"]] = caps[pl["i1"]]                         # on the grid the nearest possible: distance exactly 0
        else:
            clips[pl["k1"]] = caps[pl["i1"]] + 0.05 * near
        clips[pl["k2"]] = clips[pl["k1"]]
    return clips, caps


def ret_inputs(n_clips, n_cap, dim, family, seed=None):
    return _ret_inputs(n_clips, n_cap, dim, family, RET_SEEDS.get((n_clips, n_cap, dim, family), 0) if seed is None else seed)


def ret_d2(clips, caps, dtype):
    """d2[i][j] = |captions[i] - clips[j]|^2 (the (n_cap, n_clips, dim) block is never formed).  fp64: caption by caption.  fp32: one coordinate after
    the other into one accumulator per pair, which is the formula as l2_ranks_kernel states it; torch's own sum() adds pairwise and would stand for
    another, more accurate formula (8192 terms in sequence cost about sqrt(8192) roundings, a pairwise sum about 4)"""
    a, b = clips.to(dtype), caps.to(dtype)
    if dtype == torch.float64:
        return torch.stack([(b[i][None, :] - a).pow(2).sum(-1) for i in range(b.shape[0])])
    acc = torch.zeros(b.shape[0], a.shape[0], dtype=dtype)
    at, bt = a.t().contiguous(), b.t().contiguous()
    for k in range(a.shape[1]):
        t = bt[k][:, None] - at[k][None, :]
        acc += t * t
    return acc


def ret_decisions(d2):
    """(ranks, top1) from a matrix of squared distances, ties by index: rank = #{j : d2(i,j) < d2(i,i) or (equal and j < i)}"""
    n_cap, n_clips = d2.shape
    dii = d2[torch.arange(n_cap), torch.arange(n_cap)][:, None]
    j = torch.arange(n_clips)[None, :]
    i = torch.arange(n_cap)[:, None]
    ranks = ((d2 < dii) | ((d2 == dii) & (j < i))).sum(1).numpy().astype(np.int32)
    top1 = np.argmin(d2.numpy(), axis=1).astype(np.int32)            # numpy documents the first occurrence
    return ranks, top1


def ret_decision_margins(d2, clips):
    """from the fp64 squared distances alone: (rank, top2).
      rank  the smallest |d2(i,j) - d2(i,i)| over j != i whose clip row is not a bit-for-bit copy of clip i
      top2  the smallest gap between a row's two smallest d2; where the smallest belong to bit-for-bit equal clip rows, the gap to the next other"""
    n_cap, n_clips = d2.shape
    rank, top2 = float("inf"), float("inf")
    bits = clips.contiguous().view(torch.int32)
    for i in range(n_cap):
        same = (bits == bits[i][None, :]).all(1)
        same[i] = True
        if not bool(same.all()):
            rank = min(rank, float((d2[i][~same] - d2[i, i]).abs().min()))
        v, idx = torch.sort(d2[i], stable=True)
        k = 1
        while k < n_clips and bool((bits[idx[k]] == bits[idx[0]]).all()):
            k += 1
        if k < n_clips:
            top2 = min(top2, float(v[k] - v[0]))
    return rank, top2


@functools.lru_cache(maxsize=4)
def ret_truth(n_clips, n_cap, dim, family, seed=None):
    """(clips, caps, d2 fp64, d2 fp32, worst error of the fp32 d2): computed once, shared"""
    clips, caps = ret_inputs(n_clips, n_cap, dim, family, seed)
    d64, d32 = ret_d2(clips, caps, torch.float64), ret_d2(clips, caps, torch.float32)
    return clips, caps, d64, d32, float((d32.double() - d64).abs().max())


def ret_condition(n_clips, n_cap, dim, family, seed=None):
    """(worst fp32 error of a squared distance, rank margin, top-two margin)"""
    clips, caps, d64, d32, err = ret_truth(n_clips, n_cap, dim, family, seed)
    rank, top2 = ret_decision_margins(d64, clips)
    return err, rank, top2


def ret_condition_holds(n_clips, n_cap, dim, family, seed=None):
    err, rank, top2 = ret_condition(n_clips, n_cap, dim, family, seed)
    if family == "g":
        return err == 0.0                                            # exact in fp32: no margin is needed, ties are true ties
    return rank > COND * err and top2 > COND * err
