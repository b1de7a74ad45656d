"""Synthesis rate of the one-hot (softmax) WaveNet at the reference's size -- 24 layers / 512 residual / 512 gate / 256 skip channels, K = 256
classes, 80 conditioning channels, 8 streams, sampled (quantize=True: class form of the first conv) -- next to the mixture-of-logistics network's
chain form (VIAI_WN_PIPE=0) in the same process.  The two share the 24 layer stages; the heads differ (256 rows against 30, softmax + draw
against the mixture sampler).  Also measures the largest CDF difference to the reference on the fixture's teacher-forced probabilities
(tests/golden/wavenet_onehot_synth.npz), the quantity the sampled-run test's margins are set against.

    python tools/wn_onehot_rate.py [--out profiles/wn_onehot_rate.json] [--steps 2048]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from viai_amd.wavenet import WaveNet  # noqa: E402


def rate(net, B, T, warmup, fused, **kw):
    os.environ["VIAI_WN_PIPE"], os.environ["VIAI_WN_FUSED"] = "0", fused
    c = torch.rand(B, 80, T // 256, device="cuda")
    best = None
    for _ in range(3):
        timing = {"warmup": warmup}
        net.incremental_forward(None, c=c, T=T, timing=timing, **kw)
        us = timing["ms"] / timing["steps"] * 1e3
        best = us if best is None else min(best, us)
    return best


def cdf_error():
    """teacher-forced probabilities of the two fixture networks against the reference's: largest |CDF - CDF_ref|, per chain form"""
    from oracle import viai_oracle as O
    from oracle import wavenet_oracle as W

    class Deep(W.WNConfigDeep):
        out_channels, scalar_input = 256, False
    gold = np.load(os.path.join(ROOT, "tests", "golden", "wavenet_onehot_synth.npz"))
    res = {}
    for name, cfg, tag in (("small", W.WNConfigOneHot, "WN."), ("deep", Deep, "WNOD.")):
        B, T, K, stride, _ = (int(v) for v in gold[name + ".meta"])
        net = WaveNet(out_channels=K, layers=cfg.layers, stacks=cfg.stacks, residual_channels=cfg.residual_channels, gate_channels=cfg.gate_channels,
                      skip_out_channels=cfg.skip_out_channels, dropout=0.0, cin_channels=cfg.cin_channels, upsample_scales=list(cfg.upsample_scales),
                      scalar_input=False)
        sd = W.wavenet_state(cfg, tag)
        sd["first_conv.weight_g"] = sd["first_conv.weight_g"] * float(gold[name + ".gains"][0])
        sd["last_conv_layers.3.weight_g"] = sd["last_conv_layers.3.weight_g"] * float(gold[name + ".gains"][1])
        net.load_state_dict(sd)
        net = net.cuda().eval()
        c = O.cf_uniform("wnos.%s.c" % name, (B, cfg.cin_channels, T // 16), 0, 1).cuda()
        idx = (O.cf_uniform("wnos.%s.idx" % name, (B, T), 0, 1) * K).long().clamp(max=K - 1)
        x = torch.nn.functional.one_hot(idx, K).float().transpose(1, 2).contiguous().cuda()
        for fused in ("0", "1"):
            os.environ["VIAI_WN_FUSED"] = fused
            p = net.incremental_forward(None, c=c, T=T, test_inputs=x, softmax=True, quantize=False)[:, :, ::stride].double().cpu().numpy()
            a, b = np.cumsum(p, 1), np.cumsum(gold[name + ".p_tf"].astype(np.float64), 1)
            res["%s.fused%s" % (name, fused)] = float(np.abs(a / a[:, -1:] - b / b[:, -1:]).max())
        res[name + ".smallest_margin"] = float(gold[name + ".margins"].min())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wn_onehot_rate.json"))
    ap.add_argument("--steps", type=int, default=2048)
    ap.add_argument("--warmup", type=int, default=256)
    args = ap.parse_args()
    torch.manual_seed(1234)
    B = 8
    T = -(-(args.steps + args.warmup) // 256) * 256
    mol = WaveNet(dropout=0.0).cuda().eval()
    hot = WaveNet(out_channels=256, scalar_input=False, dropout=0.0).cuda().eval()
    out = {"network": "24 layers / 512 / 512 / 256, 80 conditioning channels", "streams": B, "timed_steps": T - args.warmup, "us_per_step": {}}
    for fused in ("1", "0"):
        a = rate(mol, B, T, args.warmup, fused)
        b = rate(hot, B, T, args.warmup, fused, return_classes=True)
        key = "fused" if fused == "1" else "plain"
        out["us_per_step"][key] = {"mol_chain": round(a, 2), "onehot_chain": round(b, 2), "ratio": round(b / a, 4),
                                   "onehot_samples_per_s": round(B * 1e6 / b, 1), "mol_samples_per_s": round(B * 1e6 / a, 1)}
        print("%s chain: mixture of logistics %.2f us per time step, one-hot %.2f us (ratio %.3f; %.0f samples/s over %d streams)"
              % (key, a, b, b / a, B * 1e6 / b, B))
    out["cdf_error_teacher_forced"] = cdf_error()
    print("largest CDF difference to the reference:", out["cdf_error_teacher_forced"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
