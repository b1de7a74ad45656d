"""Training the one-hot (softmax) WaveNet from class indices, timed against the dense one-hot path it replaces, at the reference's width:
K = 256 classes, C = 512 residual channels, B = 8 streams of T = 4096 samples.

Two paths, alternating in one process, HIP events, warm-up, median of `--reps` repetitions each:
  (a) dense: build the (B, K, T) one-hot tensor, first conv as a K = 256 1x1 conv with its weight gradient, torch cross_entropy on the
      (B, K, T) view with the mask applied in torch;
  (b) class:  `viai_class_embed_fwd / _bwd` on the class indices, `viai_masked_ce_loss` on the NHWC rows with shift = 1.
Timed: forward + backward of the input layer plus the loss (the upstream gradient of the layer and the logits are fixed tensors), and the
whole teacher-forced forward + backward of the 24-layer network, so the share of the two ends is visible.  The byte model of the two ends
is recorded next to the times.  The file's `parity` key belongs to tests/test_wavenet_onehot_train_gpu.py and is kept.

    python tools/wn_onehot_train_rate.py [--out profiles/wn_onehot_train.json] [--reps 20] [--whole-reps 20] [--dropout P]

--dropout P (default 0: the figures above) builds the network with the residual layers' dropout on (the reference trains with 0.05) under a fixed
seed; the figures of such a run, with the peak of torch.cuda.max_memory_allocated() over one class-form step, go under the file's `dropout` key
and leave the others as they are.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from viai_amd import wavenet as wn  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(paths, warmup, reps):
    """median ms per path; the paths take turns inside every repetition"""
    for _ in range(warmup):
        for fn in paths.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in paths}
    for _ in range(reps):
        for k, fn in paths.items():
            ms[k].append(timed(fn))
    return {k: statistics.median(v) for k, v in ms.items()}, {k: [min(v), max(v)] for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wn_onehot_train.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--whole-reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--length", type=int, default=4096)
    ap.add_argument("--dropout", type=float, default=0.0)
    args = ap.parse_args()
    assert args.reps >= 20 and args.whole_reps >= 20, "the median is over at least 20 repetitions"
    B, T, K, Cc = args.batch, args.length, 256, 512
    rows = B * T
    torch.manual_seed(0)
    net = wn.WaveNet(out_channels=K, layers=24, stacks=4, residual_channels=Cc, gate_channels=512, skip_out_channels=256, dropout=args.dropout,
                     cin_channels=80, upsample_scales=[4, 4, 4, 4], scalar_input=False).cuda().train()
    if args.dropout > 0:
        net.seed_dropout(0)
    first = net.first_conv
    idx = torch.randint(0, K, (B, T), device="cuda")
    c = torch.rand(B, 80, T // 256, device="cuda")
    lengths = torch.tensor([T - 1 - 14 * (b % 2) for b in range(B)], device="cuda")
    mask = wn.sequence_mask(lengths, T - 1)
    dh = torch.randn(B, 1, T, Cc, device="cuda")
    logits = torch.randn(B, 1, T, K, device="cuda").requires_grad_(True)

    def torch_loss(yh_bkt):
        ce = torch.nn.functional.cross_entropy(yh_bkt[:, :, :-1], idx[:, 1:], reduction="none")
        return (ce * mask).sum() / mask.sum()

    def ends_dense():
        net.zero_grad(set_to_none=True)
        logits.grad = None
        x = torch.nn.functional.one_hot(idx, K).float().transpose(1, 2).contiguous()
        wn.conv1d_apply(x.transpose(1, 2).unsqueeze(1).contiguous(), first).backward(dh)
        torch_loss(logits.squeeze(1).transpose(1, 2)).backward()

    def ends_class():
        net.zero_grad(set_to_none=True)
        logits.grad = None
        wn._ClassEmbed.apply(idx.to(torch.int32), wn.normed_weight(first).reshape(Cc, K), first.bias).backward(dh)
        wn.masked_cross_entropy(logits, idx, mask, shift=1).backward()

    def whole_dense():
        net.zero_grad(set_to_none=True)
        x = torch.nn.functional.one_hot(idx, K).float().transpose(1, 2).contiguous()
        torch_loss(net(x, c)).backward()

    def whole_class():
        net.zero_grad(set_to_none=True)
        wn.masked_cross_entropy(net.forward_nhwc(idx, c), idx, mask, shift=1).backward()

    # both ends agree before they are timed
    ends_dense()
    g_dense = [p.grad.clone() for p in first.parameters()] + [logits.grad.clone()]
    ends_class()
    g_class = [p.grad.clone() for p in first.parameters()] + [logits.grad.clone()]
    agree = [float((a - b).norm() / b.norm()) for a, b in zip(g_class, g_dense)]
    assert max(agree) < 2e-3, agree

    ends, ends_range = alternate({"dense": ends_dense, "class": ends_class}, args.warmup, args.reps)
    whole, whole_range = alternate({"dense": whole_dense, "class": whole_class}, 2, args.whole_reps)
    segs = wn._lib.load().viai_class_embed_bwd_segments(rows)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    whole_class()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    doc = json.load(open(args.out)) if os.path.exists(args.out) else {}
    res = doc if args.dropout == 0 else doc.setdefault("dropout", {})
    if args.dropout > 0:
        res.update({"p": args.dropout, "whole_step_class_peak_bytes": peak})
    res.update({
        "shape": {"B": B, "T": T, "K": K, "C": Cc, "rows": rows, "layers": 24},
        "method": "HIP events around forward + backward, %d warm-up, median of %d (ends) / %d (whole step) repetitions, the two paths alternating "
                  "inside every repetition, one process" % (args.warmup, args.reps, args.whole_reps),
        "ends_ms": ends, "ends_ms_min_max": ends_range, "ends_ratio_class_over_dense": ends["class"] / ends["dense"],
        "whole_step_ms": whole, "whole_step_ms_min_max": whole_range, "whole_step_ratio_class_over_dense": whole["class"] / whole["dense"],
        "ends_share_of_whole_step": {k: ends[k] / whole[k] for k in ends},
        "ends_gradients_class_vs_dense_relerr": agree,
        "byte_model": {
            "loss_per_pass": rows * K * 4,
            "loss_class": {"pass1_read": rows * K * 4, "pass2_read": rows * K * 4, "pass2_write": rows * K * 4},
            "input_layer_class": {"fwd_write_h": rows * Cc * 4, "bwd_read_dh": rows * Cc * 4, "bwd_partials_write_read": 2 * segs * K * Cc * 4,
                                  "classes_read": rows * 4},
            "input_layer_dense": {"one_hot_write_read": 2 * rows * K * 4, "fwd_read_x_write_h": rows * (K + Cc) * 4,
                                  "wgrad_read_x_dh": rows * (K + Cc) * 4},
        },
        "device": torch.cuda.get_device_name(0),
    })
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    shown = {k: res[k] for k in ("ends_ms", "ends_ratio_class_over_dense", "whole_step_ms", "whole_step_ratio_class_over_dense")}
    print(json.dumps(dict(shown, dropout=args.dropout, whole_step_class_peak_bytes=peak)))


if __name__ == "__main__":
    main()
