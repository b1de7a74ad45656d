"""What tests/test_wavenet_synth_forms_cpu.py and tests/test_wavenet_synth_forms_gpu.py share: the tiny networks of the synthesis-form tests, the list
of runs, the host-side restatement of the launch switches of csrc/wavenet.hip, the fp64 truth / fp32 yardstick of a run, the per-row measure and the
sampler-edge inputs.  No GPU and no library call in this file."""
from collections import namedtuple

import numpy as np
import torch

from oracle import viai_oracle as O
from oracle import wavenet_oracle as W

MARGIN = 4.0                 # tests/test_wavenet_train_kernels_gpu.py: another, equally valid fp32 summation order
LOG_SCALE_MIN = -7.0

# ------------------------------------------------------------------------------------------------------------------------------ the networks
# name: (C, G, S, cin, layers, stacks, out_channels, scalar_input, gin)      H = G / 2.  Conditioning arrives at the sample rate (no up-sampling stack).
NETS = {
    "floor":      (4, 8, 4, 4, 2, 1, 30, True, -1),         # smallest legal step; one 16-byte chunk per reduction
    "ragged":     (100, 136, 36, 20, 3, 1, 30, True, -1),   # 3C = 300, H = 68: loops with remainders; C + S = 136 rows in 4-row blocks
    "rows-head":  (32, 128, 32, 80, 4, 2, 30, True, -1),    # fused form, S <= H
    "fused-head": (32, 32, 32, 80, 4, 2, 30, True, -1),     # fused form, S > H
    "wide-skip":  (64, 64, 260, 80, 2, 1, 30, True, -1),    # S > 256: fused form refused, generic head
    "wide-gate":  (16, 520, 16, 4, 2, 1, 30, True, -1),     # G / 2 > 256: fused form refused
    "deep":       (8, 16, 8, 4, 6, 1, 30, True, -1),        # dilations 1 .. 32, ring of 65 slots
    "global":     (12, 24, 12, 4, 2, 1, 30, True, 4),       # g_add, with and without local conditioning
    "onehot256":  (12, 24, 12, 4, 2, 1, 256, False, -1),    # categorical head, K = four waves
    "onehot68":   (12, 24, 12, 4, 2, 1, 68, False, -1),     # two waves, the second ragged
    "onehot12":   (12, 24, 12, 4, 2, 1, 12, False, -1),     # less than one wave
    "onehot4":    (12, 24, 12, 4, 2, 1, 4, False, -1),
    "single":     (12, 24, 12, 4, 1, 1, 30, True, -1),      # n == 1: the first skip is also the last, no next ring
    "single12":   (12, 24, 12, 4, 1, 1, 12, False, -1),
}
N_SPEAKERS = 3


def make_cfg(name):
    C, G, S, cin, layers, stacks, out, scalar, gin = NETS[name]
    return type("WNSynth_" + name.replace("-", "_"), (W.WNConfig,), dict(
        out_channels=out, layers=layers, stacks=stacks, residual_channels=C, gate_channels=G, skip_out_channels=S, cin_channels=cin,
        upsample_scales=(), scalar_input=scalar, gin_channels=gin, n_speakers=N_SPEAKERS if gin > 0 else None))


def state(name):
    """weight-normalised like the reference (oracle.wavenet_state), own tags; the one-hot networks get the sharpening gains of the golden fixture's
    generator (first conv x 4, output layer x 12) so that which class is fed matters"""
    cfg = make_cfg(name)
    sd = W.wavenet_state(cfg, "WNSF.%s." % name)
    if not cfg.scalar_input:
        sd["first_conv.weight_g"] = sd["first_conv.weight_g"] * 4.0
        sd["last_conv_layers.3.weight_g"] = sd["last_conv_layers.3.weight_g"] * 12.0
    return cfg, sd


def dilations(name):
    _, _, _, _, layers, stacks, _, _, _ = NETS[name]
    return [2 ** (i % (layers // stacks)) for i in range(layers)]


def length(name):
    """at least twice the longest ring (2 d + 1 slots) plus 5: every ring wraps twice and T is no multiple of anything; 24 up to d = 4, 140 for d = 32"""
    ring = 2 * max(dilations(name)) + 1
    T = 24 if ring <= 9 else 140
    assert T >= 2 * ring + 5
    return T


# --------------------------------------------------------------------------------------------------------------------------------- the runs
# (network, form, B, options).  form: "unfused" = chain with VIAI_WN_FUSED=0, "fused" = chain as the library chooses (fused where wn_fused_ok), "graph" =
# use_graph=True (fused where wn_fused_ok), "graph-unfused" = use_graph=True with VIAI_WN_FUSED=0.  options: "nocond" (c = None), "dense" (input_form="dense"),
# "mask" (forced= with a mixed mask).  B in 1, 2, 4, 8 occurs for every form family; no full product.
Run = namedtuple("Run", "net form B opts")
RUNS = [Run(*r) for r in [
    ("floor", "unfused", 1, ()), ("floor", "fused", 8, ()), ("floor", "graph", 4, ()),
    ("ragged", "unfused", 2, ()), ("ragged", "fused", 4, ()), ("ragged", "graph", 1, ()), ("ragged", "graph-unfused", 8, ()),
    ("ragged", "unfused", 4, ("mask",)), ("ragged", "fused", 2, ("mask",)), ("ragged", "graph", 8, ("mask",)),
    ("rows-head", "unfused", 4, ()), ("rows-head", "fused", 1, ()), ("rows-head", "graph", 8, ()),
    ("fused-head", "unfused", 8, ()), ("fused-head", "fused", 2, ()), ("fused-head", "graph", 4, ()),
    ("wide-skip", "unfused", 2, ()), ("wide-skip", "fused", 1, ()), ("wide-skip", "graph", 8, ()),
    ("wide-gate", "unfused", 4, ()), ("wide-gate", "fused", 8, ()), ("wide-gate", "graph", 1, ()),
    ("deep", "unfused", 1, ()), ("deep", "fused", 2, ()), ("deep", "graph", 4, ()),
    ("global", "unfused", 8, ()), ("global", "fused", 1, ()), ("global", "graph", 2, ()),
    ("global", "unfused", 2, ("nocond",)), ("global", "fused", 4, ("nocond",)), ("global", "graph", 8, ("nocond",)),
    ("onehot256", "unfused", 1, ()), ("onehot256", "fused", 8, ("dense",)), ("onehot256", "graph", 2, ()),
    ("onehot68", "unfused", 2, ("dense",)), ("onehot68", "fused", 4, ()), ("onehot68", "graph", 1, ("dense",)),
    ("onehot68", "unfused", 8, ("mask",)), ("onehot68", "fused", 2, ("mask",)),
    ("onehot12", "unfused", 4, ()), ("onehot12", "fused", 2, ("dense",)), ("onehot12", "graph", 8, ()),
    ("onehot4", "unfused", 8, ("dense",)), ("onehot4", "fused", 1, ()), ("onehot4", "graph", 4, ()),
    ("single", "unfused", 2, ()), ("single", "fused", 8, ()), ("single", "graph", 1, ()),
    ("single12", "unfused", 4, ()), ("single12", "fused", 1, ("dense",)), ("single12", "graph", 2, ()),
    ("floor", "unfused", 1, ("nocond",)), ("fused-head", "fused", 8, ("nocond",)),
]]


def run_id(r):
    return "-".join((r.net, r.form, "B%d" % r.B) + tuple(r.opts))


def switches(r):
    """Which side of every switch of a synthesis step a run takes, from the shapes alone: the host-side restatement of wavenet_synth.incremental_forward's
    `fuse`, wn_fused_ok, wn_step_impl / wn_step_fused_impl, wn_cat_head and wn_cat_dense_at (csrc/wavenet.hip).  Returns a dict of switch -> side and the
    list of kernels launched per time step, in launch order."""
    C, G, S, cin, layers, stacks, out, scalar, gin = NETS[r.net]
    H = G // 2
    env_fused = r.form in ("fused", "graph")
    fused = env_fused and S <= 256 and out <= 256 and H <= 256                      # wavenet_synth.py `fuse` (staged weights present) == wn_fused_ok
    device_t = r.form.startswith("graph")
    cat = not scalar
    # teacher-forced one-hot rows through the K-long product; under a mask the fed-back probabilities are dense rows, the forced streams classes ("mixed")
    dense = cat and ("dense" in r.opts or "mask" in r.opts)
    sw = {"fused": fused, "refused_by": None if fused or not env_fused else ("S" if S > 256 else "H"), "NB": r.B, "device_t": device_t,
          "categorical": cat, "cat_first": ("mixed" if "mask" in r.opts else "dense" if dense else "class") if cat else None, "mask": "mask" in r.opts,
          "cond": ("local" if "nocond" not in r.opts else "") + ("+global" if gin > 0 else ""),
          "n": "1" if layers == 1 else ("2" if layers == 2 else ">2"), "head": None}
    NB = "<%d>" % r.B
    k = []
    if fused:
        if device_t:
            k.append("wn_tick_kernel")
        if dense:
            k.append("wn_cat_first_kernel" + NB + "(dense_only)")
        k += ["wn_stage_kernel" + ("<%d,%s>" % (r.B, "CAT" if (cat and l == 0) else "-")) for l in range(layers)]
        if cat:
            k += ["wn_head_rows_kernel" + NB, "wn_cat_rows_kernel" + NB, "wn_cat_rows_kernel" + NB, "wn_cat_sample_kernel"]
            sw["head"] = "cat"
        elif S <= H:
            k += ["wn_head_rows_kernel" + NB, "wn_head_rows_kernel" + NB, "wn_head_sample_kernel"]
            sw["head"] = "rows+sample"
        else:
            k.append("wn_head_fused_kernel")
            sw["head"] = "head_fused"
    else:
        if cat:
            k += (["wn_tick_kernel"] if device_t else []) + ["wn_cat_first_kernel" + NB]
        else:
            k.append("wn_first_kernel")
        k += ["wn_gate_kernel" + NB, "wn_out_kernel" + NB] * layers
        if cat:
            k += ["wn_cat_rows_kernel" + NB, "wn_cat_rows_kernel" + NB, "wn_cat_sample_kernel"]
            sw["head"] = "cat"
        elif S <= 256 and out <= 256:
            k.append("wn_head_kernel")
            sw["head"] = "head"
        else:
            k.append("wn_head_generic_kernel")
            sw["head"] = "head_generic"
    return sw, k


# ------------------------------------------------------------------------------------------------------------------------------- the inputs
def inputs(r, T=None):
    """every stream its own conditioning, input, speaker and uniforms (closed-form, CPU, fp32)"""
    C, G, S, cin, layers, stacks, out, scalar, gin = NETS[r.net]
    T = length(r.net) if T is None else T
    tag = "wnsf.%s.%d." % (r.net, r.B)
    d = {"T": T}
    d["c"] = None if "nocond" in r.opts else O.cf_uniform(tag + "c", (r.B, cin, T), 0, 1)
    d["g"] = (torch.arange(r.B) % N_SPEAKERS).reshape(r.B, 1) if gin > 0 else None
    if scalar:
        d["x"] = O.cf_uniform(tag + "x", (r.B, 1, T), -1, 1)
        d["u1"], d["u2"] = O.cf_uniform(tag + "u1", (r.B, T, out // 3), 1e-5, 1 - 1e-5), O.cf_uniform(tag + "u2", (r.B, T), 1e-5, 1 - 1e-5)
    else:
        d["cls"] = (O.cf_uniform(tag + "idx", (r.B, T), 0, 1) * out).long().clamp(max=out - 1)
        d["x"] = torch.nn.functional.one_hot(d["cls"], out).float().transpose(1, 2).contiguous()
        d["u1"], d["u2"] = None, O.cf_uniform(tag + "u", (r.B, T), 0, 1)
    d["mask"] = (O.cf_uniform(tag + "m", (r.B, T), 0, 1) < 0.6) if "mask" in r.opts else None     # mixed: ~ 60 % of the steps forced, per stream
    return d


def effective_inputs(d, fed, scalar, K):
    """the input every step of a masked or free-running GPU run actually consumed: d["x"] where the step was forced (d["mask"], or the prefix
    of d["n_prefix"] steps), else what the GPU put out one step earlier (`fed`, (B, 1 or K, T)); at t = 0 the start value (0 / class 127, or 0 where K <= 127)"""
    B, T = fed.shape[0], d["T"]
    fed = torch.as_tensor(fed).detach().float().cpu()
    start = torch.zeros(B, 1, 1) if scalar else torch.nn.functional.one_hot(torch.full((B, 1), 127 if K > 127 else 0), K).float().transpose(1, 2)
    prev = torch.cat((start, fed[:, :, :T - 1]), 2)
    m = d["mask"] if d.get("mask") is not None else (torch.arange(T) < d["n_prefix"]).reshape(1, T).expand(B, T)
    x = torch.zeros_like(prev)
    n = d["x"].shape[-1]
    x[:, :, :n] = d["x"]
    return torch.where(m.reshape(B, 1, T), x, prev)


def oracle_logits(name, sd, d, x, dtype, **kw):
    """logits (B, T, out) of the ring algorithm teacher-forced on x over all T steps"""
    cfg = make_cfg(name)
    _, lg = W.incremental_forward_ring(sd, d["c"], d["T"], d["u1"], d["u2"], cfg, test_inputs=x, log_scale_min=LOG_SCALE_MIN, g=d["g"],
                                       return_logits=True, dtype=dtype, softmax=False, quantize=False, **kw)
    return lg.transpose(1, 2).contiguous()


# ------------------------------------------------------------------------------------------------------------------------------ the measure
def row_errors(got, truth):
    """(B, T) errors of rows (stream, time step): max_k |got - truth| / max(max_k |truth|, floor), floor = the run's median row maximum"""
    got, truth = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(truth).detach().double().cpu()
    assert got.shape == truth.shape and got.dim() == 3, (got.shape, truth.shape)
    rmax = truth.abs().amax(-1)
    floor = rmax.median()
    return (got - truth).abs().amax(-1) / torch.maximum(rmax, floor)


def worst_row(got, truth):
    """worst row error and where: (error, stream, step, channel)"""
    e = row_errors(got, truth)
    b, t = divmod(int(e.argmax()), e.shape[1])
    ch = int((torch.as_tensor(got).detach().double().cpu()[b, t] - torch.as_tensor(truth).double()[b, t]).abs().argmax())
    return float(e[b, t]), b, t, ch


def frobenius(got, truth):
    """the aggregate measure of the older tests: relative L2 error over the whole tensor"""
    got, truth = torch.as_tensor(got).detach().double().cpu().reshape(-1), torch.as_tensor(truth).detach().double().cpu().reshape(-1)
    return float((got - truth).norm() / truth.norm())


def check_rows(got, truth, yard, what):
    """worst row of `got` against the fp64 truth under MARGIN x the worst row of the fp32 restatement `yard`; prints both first"""
    e, b, t, ch = worst_row(got, truth)
    y = worst_row(yard, truth)[0]
    print("%-44s worst row %.3e (stream %d, step %d, channel %d)   fp32 torch %.3e   ratio %.2f" % (what, e, b, t, ch, y, e / y if y > 0 else float("inf")))
    assert e <= MARGIN * y, "%s: stream %d, step %d, channel %d: row error %.3e > %g x %.3e" % (what, b, t, ch, e, MARGIN, y)
    return e, y


# ---------------------------------------------------------------------------------------------------------------------- sampler edges: mixture
NR_MIX = 10
MEANS = torch.arange(NR_MIX, dtype=torch.float32) * 0.15 - 0.675            # 0.15 apart: a wrong component shows
MOL_T = 24


def mol_row(logit, log_scale):
    return torch.cat((torch.as_tensor(logit, dtype=torch.float32).expand(NR_MIX).clone(), MEANS, torch.as_tensor(log_scale, dtype=torch.float32).expand(NR_MIX).clone()))


def mol_edge_cases(B=1, T=MOL_T):
    """name -> (row (30,), log_scale_min, u1 (B, T, 10), u2 (B, T), clipped).  Injected uniforms differ per stream and step: T steps are T cases.
    clamp-*: every log-scale is float32(-5), log_scale_min just above it (the clamp acts), exactly it, and just below (it does not).
    clip: log-scale 0, u2 alternating 1e-5 / 1 - 1e-5: x = mean -/+ 11.5 leaves [-1, 1] on either side (the component does not show in a clipped value).
    gumbel: equal component logits, u1 with the winner's Gumbel term >= 0.05 ahead of the runner-up (no tie, fp64 lead >= 1e-3).
    dominant: one logit + 30 against Gumbel terms of at most 11.5."""
    rnd = O.cf_uniform("wnsf.mol.logit", (NR_MIX,), -1, 1)
    u1 = O.cf_uniform("wnsf.mol.u1", (B, T, NR_MIX), 1e-5, 1 - 1e-5)
    u2 = O.cf_uniform("wnsf.mol.u2", (B, T), 1e-3, 1 - 1e-3)                 # |logit(u2)| exp(-5) < 0.047 < 0.075: the component shows
    ls = float(torch.tensor(-5.0, dtype=torch.float32))
    cases = {
        "clamp-below": (mol_row(rnd, -5.0), -4.9, u1, u2, False),
        "clamp-at": (mol_row(rnd, -5.0), ls, u1, u2, False),
        "clamp-above": (mol_row(rnd, -5.0), -5.1, u1, u2, False),
    }
    alt = torch.where((torch.arange(T).reshape(1, T) + torch.arange(B).reshape(B, 1)) % 2 == 0, torch.tensor(1e-5), torch.tensor(1 - 1e-5)).float()
    cases["clip"] = (mol_row(rnd, 0.0), LOG_SCALE_MIN, u1, alt, True)
    ug = O.cf_uniform("wnsf.mol.ug", (B, T, NR_MIX), 0.05, 0.80)
    win = (torch.arange(T).reshape(1, T) * 3 + torch.arange(B).reshape(B, 1)) % NR_MIX
    ug.scatter_(2, win.unsqueeze(-1), 0.85)                                   # -log(-log(.85)) = 1.817, of .80: 1.500
    cases["gumbel"] = (mol_row(0.25, -5.0), LOG_SCALE_MIN, ug, u2, False)
    dom = rnd.clone()
    dom[7] += 30.0
    cases["dominant"] = (mol_row(dom, -5.0), LOG_SCALE_MIN, u1, u2, False)
    return cases


def mol_truth(row, lsm, u1, u2, dtype):
    """oracle.mol_sample on the constant row: (values (B, T), component (B, T))"""
    B, T = u2.shape
    y = row.to(dtype).reshape(1, 3 * NR_MIX, 1).expand(B, 3 * NR_MIX, T)
    v = W.mol_sample(y, u1.to(dtype), u2.to(dtype), lsm)
    score = row[:NR_MIX].to(dtype) - torch.log(-torch.log(u1.to(dtype)))
    return v, score.argmax(-1), score


def component_of(values):
    """the component a value came from: the nearest mean (valid while |x - mean| < 0.075)"""
    return torch.round((torch.as_tensor(values).double().cpu() - float(MEANS[0])) / 0.15).long().clamp(0, NR_MIX - 1)


# ------------------------------------------------------------------------------------------------------------------ sampler edges: categorical
CAT_KS = (256, 68, 12, 4)
EDGE_OFF = 3e-5
EDGE_KEEP = 1e-5             # a draw whose u lies within this of an fp64 class edge decides nothing and is dropped


def cat_rows(K):
    """flat, random and peaked (one logit + 40, mid-row) logits rows of K classes, fp32"""
    rnd = O.cf_uniform("wnsf.cat.row%d" % K, (K,), -2, 2)
    peak = O.cf_uniform("wnsf.cat.peak%d" % K, (K,), -1, 1)
    peak[K // 2] += 40.0
    return {"flat": torch.zeros(K), "random": rnd, "peaked": peak}


def cat_cdf64(row):
    p = torch.softmax(row.double(), 0)
    cdf = torch.cumsum(p, 0)
    return (cdf / cdf[-1]).numpy()


def cat_edge_uniforms(row):
    """(u (n,) fp32, class (n,), dropped) for one logits row: u at 0, EDGE_OFF below and above several class edges (cdf[k], k <= K - 2: the first, the last,
    some between), and 1 - 1e-7.  Every u is the fp32 number that reaches the kernel; its class is the fp64 inverse cdf of that number.  A candidate outside
    [0, 1) cannot be drawn and is not constructed; at the peaked row the edges gather at 0 and at 1, so 0 and 1 - 1e-7 are within EDGE_KEEP of an edge wherever
    the peak sits and are not constructed there either.  `dropped` counts constructed draws within EDGE_KEEP of an edge: the construction makes it 0."""
    K = row.numel()
    cdf = cat_cdf64(row)
    edges = cdf[:K - 1]
    ks = sorted({0, 1, (K - 1) // 3, (K - 1) // 2, K // 2, K - 3, K - 2} & set(range(K - 1)))
    cand = []
    clustered = float(np.diff(edges).min()) < 4 * EDGE_OFF if K > 2 else False
    if not clustered:
        cand += [0.0, 1.0 - 1e-7]
    for k in ks:
        cand += [float(edges[k]) - EDGE_OFF, float(edges[k]) + EDGE_OFF]
    j = (K - 1) // 2
    cand.append(0.5 if clustered else 0.5 * (float(edges[j - 1]) + float(edges[j])))      # and one draw inside a class
    u = np.array([c for c in cand if 0.0 <= np.float32(c) < 1.0], dtype=np.float32)
    dist = np.abs(u.astype(np.float64)[:, None] - edges[None, :]).min(1)
    cls = np.minimum((cdf[None, :] <= u.astype(np.float64)[:, None]).sum(1), K - 1)
    return torch.from_numpy(u), torch.from_numpy(cls), int((dist <= EDGE_KEEP).sum())
