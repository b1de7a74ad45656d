#!/usr/bin/env python
"""Time of TV-L1 optical flow (viai_amd.optical_flow, csrc/optical_flow.hip) per pair of frames at 480 x 640 with the default parameters
(5 levels, 5 warps, 30 iterations), for `iters_per_launch` = 1 (the plain form: one launch per iteration) and for the fused forms, from the
same build in the same process.  The K = 1 figure is the yardstick for what running several iterations per launch over an LDS tile buys.

Per K and per number of pairs in the call: stream time of one `viai_optical_flow` call from device events (median, best and worst of `--reps`
calls after warm-up calls; the workspace is made once), microseconds per pair, the launches of the call, and the byte model of DESIGN.md
11.2o: an iteration launch reads the six evolving planes and the four constants and writes the six planes, 64 bytes per pixel of the level
(the halo a block reads on top of its tile is not in the model, it is what the fused form pays), so fusing K iterations divides the model's
bytes by K.  Every K is checked to give the bits of K = 1 before it is timed.

No rate here is a threshold: the figures go into DESIGN.md 11.2o so that a later change has something to beat.

    python tools/optical_flow_rate.py [--pairs 1 32] [--reps 10] [--json profiles/optical_flow_rate.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps, warm=2):
    """stream seconds per call"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t = []
    for _ in range(reps):
        ev0.record()
        fn()
        ev1.record()
        torch.cuda.synchronize()
        t.append(ev0.elapsed_time(ev1) * 1e-3)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--pairs", type=int, nargs="+", default=[1, 32])
    ap.add_argument("--ks", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "optical_flow_rate.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("optical_flow_rate: no GPU; a time is a measurement on the device or nothing")
    from viai_amd import _lib
    from viai_amd.ops import _stream
    from viai_amd.optical_flow import ITERS_PER_LAUNCH, PARAMS
    lib = _lib.load()
    H, W = a.height, a.width
    p = PARAMS
    S = int(lib.viai_optical_flow_levels(H, W, p["scales"]))
    shapes = [(H, W)]
    for _ in range(S - 1):
        shapes.append(((shapes[-1][0] + 1) // 2, (shapes[-1][1] + 1) // 2))
    px = sum(h * w for h, w in shapes)
    result = {"tool": "optical_flow_rate", "device": torch.cuda.get_device_name(0), "height": H, "width": W, "levels": S, "reps": a.reps,
              "params": p, "default_iters_per_launch": ITERS_PER_LAUNCH, "runs": []}
    print("%d x %d, %d levels, %d warps, %d iterations; median (best - worst) of %d calls" % (H, W, S, p["warps"], p["iterations"], a.reps))
    yy, xx = torch.meshgrid(torch.arange(H, device="cuda", dtype=torch.float32), torch.arange(W, device="cuda", dtype=torch.float32), indexing="ij")
    for P in a.pairs:
        # a texture that moves by (1.5, -0.75) px per frame: the kernels' time does not depend on the values, the check below does
        frames = torch.stack([(127.5 + 60 * torch.sin((xx - 1.5 * n) / 5.0) * torch.cos((yy + 0.75 * n) / 7.0) +
                               40 * torch.sin((xx - 1.5 * n + 2 * (yy + 0.75 * n)) / 11.0)).round().clamp(0, 255).to(torch.uint8)
                              for n in range(P + 1)]).contiguous()
        ws = torch.empty(int(lib.viai_optical_flow_ws_bytes(P, H, W, p["scales"])) // 4 + 1, dtype=torch.float32, device="cuda")
        flow = torch.empty((P, 2, H, W), dtype=torch.float32, device="cuda")
        first = None
        for K in a.ks:
            def call():
                _lib.check(lib.viai_optical_flow(frames.data_ptr(), H * W, P + 1, H, W, 1, 0, p["tau"], p["lam"], p["theta"], p["scales"], p["warps"],
                                                 p["iterations"], K, flow.data_ptr(), ws.data_ptr(), _stream()), "viai_optical_flow")
            call()
            torch.cuda.synchronize()
            if first is None:
                first = flow.clone()
            assert torch.equal(flow.view(torch.int32), first.view(torch.int32)), "K = %d differs from K = %d" % (K, a.ks[0])
            t = timed(call, a.reps)
            med = statistics.median(t)
            launches = int(lib.viai_optical_flow_launches(H, W, p["scales"], p["warps"], p["iterations"], K))
            iter_launches = S * p["warps"] * -(-p["iterations"] // K)
            model = 64 * px * P * p["warps"] * -(-p["iterations"] // K)
            e = {"pairs": P, "iters_per_launch": K, "launches": launches, "iteration_launches": iter_launches,
                 "us_median": round(med * 1e6, 1), "us_min": round(min(t) * 1e6, 1), "us_max": round(max(t) * 1e6, 1),
                 "us_per_pair": round(med * 1e6 / P, 1), "us_per_launch": round(med * 1e6 / launches, 2),
                 "iteration_bytes_model": int(model), "model_gb_per_s": round(model / med / 1e9, 1), "workspace_bytes": int(ws.numel() * 4),
                 "mean_flow": [round(float(flow[:, 0, 8:-8, 8:-8].mean()), 4), round(float(flow[:, 1, 8:-8, 8:-8].mean()), 4)]}
            result["runs"].append(e)
            print("  pairs %3d  K %d | %4d launches | %10.1f us (%.1f - %.1f) | %9.1f us per pair | %6.2f us per launch | model %7.1f GB/s"
                  % (P, K, launches, e["us_median"], e["us_min"], e["us_max"], e["us_per_pair"], e["us_per_launch"], e["model_gb_per_s"]))
    print(json.dumps(result, sort_keys=True))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(result, f, sort_keys=True, indent=1)


if __name__ == "__main__":
    main()
