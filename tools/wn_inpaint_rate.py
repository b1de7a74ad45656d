"""Wall time of `inpaint_waveform` at the reference's size -- 24 layers / 512 residual / 512 gate / 256 skip channels, 80 conditioning channels,
hop 256, 8 streams -- on a 208-frame clip (53 248 samples) with a 52-frame gap per stream drawn by `make_time_mask`, next to the only way to get
those samples without it: ONE prefix-forced `incremental_forward` over the whole clip (teacher-forced up to the first gap of the batch, free from
there on).  The inpainting call runs receptive field + gap = 505 + 13 312 steps of the chain form; the whole-clip call takes whatever form the
library picks for it (the pipelined one where the device offers it; `--chain` pins the chain of launches).  Expect roughly (R + gap) / n of the
whole-clip time when both run the same form.

    python tools/wn_inpaint_rate.py [--out profiles/wn_inpaint_rate.json] [--frames 208] [--gap 52] [--chain]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from viai_amd.model import make_time_mask  # noqa: E402
from viai_amd.wavenet import WaveNet, gaps_from_mask, inpaint_waveform  # noqa: E402


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wn_inpaint_rate.json"))
    ap.add_argument("--frames", type=int, default=208)
    ap.add_argument("--gap", type=int, default=52)
    ap.add_argument("--chain", action="store_true", help="VIAI_WN_PIPE=0: the full-clip call runs the chain of launches too")
    args = ap.parse_args()
    if args.chain:
        os.environ["VIAI_WN_PIPE"] = "0"
    torch.manual_seed(1234)
    B, hop = 8, 256
    n = args.frames * hop
    net = WaveNet(dropout=0.0).cuda().eval()
    R = net.receptive_field
    wav = (torch.rand(B, n, device="cuda") * 2 - 1) * 0.5
    c = torch.rand(B, 80, args.frames, device="cuda")
    gs, gl = gaps_from_mask(make_time_mask(B, args.frames, args.gap, generator=torch.Generator().manual_seed(7)))
    L = R + args.gap * hop
    u = (torch.empty(B, L, 10, device="cuda").uniform_(1e-5, 1 - 1e-5), torch.empty(B, L, device="cuda").uniform_(1e-5, 1 - 1e-5))
    inpaint_waveform(net, wav[:, :8 * hop], c[:, :, :8], 2, 1)                         # warm-up: library load, first launches
    t_inpaint = wall(lambda: inpaint_waveform(net, wav, c, gs, gl, uniforms=u))
    # today's way: the clip's samples as a teacher-forced prefix up to the first gap, free-running from there to the end of the clip
    first = int(gs.min()) * hop
    timing = {"warmup": 0}
    t_full = wall(lambda: net.incremental_forward(None, c=c, T=n, test_inputs=wav[:, :first].unsqueeze(1).contiguous(), timing=timing))
    out = {"network": "24 layers / 512 / 512 / 256, 80 conditioning channels, hop %d" % hop, "streams": B, "clip_samples": n,
           "gap_samples": args.gap * hop, "receptive_field": R, "window_steps": L,
           "inpaint_waveform_s": round(t_inpaint, 3), "inpaint_form": "chain (fused)" if os.environ.get("VIAI_WN_FUSED", "1") != "0" else "chain",
           "full_clip_incremental_forward_s": round(t_full, 3), "full_clip_form": timing.get("form", "chain"),
           "ratio": round(t_inpaint / t_full, 4), "steps_ratio": round(L / n, 4)}
    print("inpaint_waveform: %.3f s for %d window steps (%s); whole clip, prefix-forced: %.3f s for %d steps (%s); ratio %.3f, steps ratio %.3f"
          % (t_inpaint, L, out["inpaint_form"], t_full, n, out["full_clip_form"], out["ratio"], out["steps_ratio"]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
