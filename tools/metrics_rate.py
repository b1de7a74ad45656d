#!/usr/bin/env python
"""Time per call of the inpainting metrics (viai_amd.metrics, csrc/metrics.hip) at the native shape: B = 8 clips of n = 65 536 samples with an
8192-sample gap each at a start that is no multiple of anything, and 80 x 259 mels with a mask of damaged frames.  Per function: wall time of the
whole Python call (argument checks, the upload of the gap bounds, allocations, two launches, a synchronise), stream time of the same call (events),
and beside them the bytes the kernels must read from memory, from the shapes.  At this size the calls are a few launches' worth of fixed cost; the
bytes column says how little there is to read, not what the kernels can sustain.  No threshold: the figures go into DESIGN.md 11.2k.

    python tools/metrics_rate.py [--streams 8] [--samples 65536] [--gap 8192] [--frames 259] [--reps 50] [--json PATH]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps):
    """(wall seconds, stream seconds) per call, `reps` of each after three warm-up calls"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        wall.append(time.perf_counter() - t0)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    stream = []
    for _ in range(reps):
        ev0.record()
        fn()
        ev1.record()
        torch.cuda.synchronize()
        stream.append(ev0.elapsed_time(ev1) * 1e-3)
    return wall, stream


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=8)
    ap.add_argument("--samples", type=int, default=65536)
    ap.add_argument("--gap", type=int, default=8192)
    ap.add_argument("--mels", type=int, default=80)
    ap.add_argument("--frames", type=int, default=259)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--json", default=None, help="also write the figures to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("metrics_rate: no GPU; a time is a measurement on the device or nothing")
    from viai_amd import metrics as M
    B, n, F, T, win = a.streams, a.samples, a.mels, a.frames, 11
    g = torch.Generator().manual_seed(0)
    ref = (torch.rand(B, n, generator=g) * 1.8 - 0.9).cuda()
    est = (0.9 * ref.cpu() + 0.1 * (torch.rand(B, n, generator=g) * 1.8 - 0.9)).cuda()
    starts = [10001 + 1111 * b for b in range(B)]
    g0, glen = torch.tensor(starts), torch.full((B,), a.gap)
    mel_r = torch.rand(B, 1, F, T, generator=g).cuda()
    mel_e = (mel_r.cpu() + 0.1 * (torch.rand(B, 1, F, T, generator=g) - 0.5)).clamp(0, 1).cuda()
    mask = torch.ones(B, 1, 1, T)
    d0, dn = T // 3, 36                                                   # 36 damaged frames: an 8192-sample gap at fft 1024 / hop 256, widened
    mask[..., d0:d0 + dn] = 0
    mask = mask.cuda()
    # bytes the kernels must read: both inputs over the region, the mask once; SSIM's region is the damaged centres' windows (dn + win - 1 frames)
    need = {
        "wave_gap_stats": 2 * 4 * B * a.gap,
        "mel_frame_stats[damaged]": 2 * 4 * B * F * dn + 4 * B * T,
        "mel_frame_stats[all]": 2 * 4 * B * F * T,
        "mel_ssim[damaged]": 2 * 4 * B * F * (dn + win - 1) + 4 * B * T,
        "mel_ssim[all]": 2 * 4 * B * F * T,
    }
    calls = {
        "wave_gap_stats": lambda: M.wave_gap_stats(ref, est, g0, glen),
        "mel_frame_stats[damaged]": lambda: M.mel_frame_stats(mel_r, mel_e, mask, "damaged"),
        "mel_frame_stats[all]": lambda: M.mel_frame_stats(mel_r, mel_e, None, "all"),
        "mel_ssim[damaged]": lambda: M.mel_ssim(mel_r, mel_e, mask, "damaged"),
        "mel_ssim[all]": lambda: M.mel_ssim(mel_r, mel_e, None, "all"),
    }
    print("metrics at B = %d, n = %d, gap %d, mel %d x %d, %d damaged frames, win %d; median (best - worst) of %d calls"
          % (B, n, a.gap, F, T, dn, win, a.reps))
    result = {"tool": "metrics_rate", "streams": B, "samples": n, "gap": a.gap, "mels": F, "frames": T, "damaged_frames": dn, "reps": a.reps,
              "device": torch.cuda.get_device_name(0), "calls": {}}
    for name, fn in calls.items():
        wall, stream = timed(fn, a.reps)
        us = lambda v: "%.1f (%.1f - %.1f)" % (statistics.median(v) * 1e6, min(v) * 1e6, max(v) * 1e6)
        print("  %-26s wall %s us | stream %s us | must read %.3f MB"
              % (name, us(wall), us(stream), need[name] / 1e6))
        result["calls"][name] = {"wall_us_median": round(statistics.median(wall) * 1e6, 2), "wall_us_min": round(min(wall) * 1e6, 2),
                                 "stream_us_median": round(statistics.median(stream) * 1e6, 2), "stream_us_min": round(min(stream) * 1e6, 2),
                                 "bytes_needed": need[name]}
    print(json.dumps(result, sort_keys=True))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(result, f, sort_keys=True, indent=1)


if __name__ == "__main__":
    main()
