#!/usr/bin/env python
"""Time per call of the polyphase resampler (viai_amd.wav_resample, csrc/wav_resample.hip) at B = 8 clips of n = 65 536 x 441 / 160 = 180 633
samples: 44.1 kHz -> 16 kHz on the clip, and 16 kHz -> 44.1 kHz on its result.  Per direction: wall time of the whole Python call (checks, the
allocation, one launch, a synchronise), stream time of the same call (events), and the bytes the call must move -- every input sample read once,
every output written once -- per second of stream time.  Beside it what a plain copy reaches on the same machine (tools/probes/hbm_stream.py,
run as a child process), which is what those bytes would cost if the filter were free.  No threshold: the figures go into DESIGN.md 11.2l.

    python tools/wav_resample_rate.py [--streams 8] [--samples 180633] [--reps 50] [--json profiles/wav_resample_rate.json]
"""
import argparse
import json
import os
import statistics
import subprocess
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


def copy_rate():
    """(TB/s of the copy line, the probe's whole output); (None, text) when the probe printed no such line"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "probes", "hbm_stream.py")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=300)
    for line in r.stdout.splitlines():
        f = line.split()
        if f and f[0] == "copy" and f[-1] == "TB/s":
            return float(f[-2]), r.stdout
    return None, r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=8)
    ap.add_argument("--samples", type=int, default=65536 * 441 // 160)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "wav_resample_rate.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("wav_resample_rate: no GPU; a time is a measurement on the device or nothing")
    from viai_amd.wav_resample import Resampler
    B, n = a.streams, a.samples
    down, up = Resampler(44100, 16000), Resampler(16000, 44100)
    g = torch.Generator().manual_seed(0)
    hi = (torch.rand(B, n, generator=g) * 1.8 - 0.9).cuda()
    lo = down(hi)
    m = lo.size(1)
    back = torch.empty(B, up.out_len(m), device="cuda")
    gap0, gap1 = n // 3, n // 3 + 22050                                  # half a second at 44.1 kHz, written into an existing clip
    calls = {
        "44.1k->16k": (lambda: down(hi), 4 * B * (n + m), down),
        "16k->44.1k": (lambda: up(lo, out=back), 4 * B * (m + back.size(1)), up),
        "16k->44.1k[gap]": (lambda: up(lo, out=back, window=(gap0, gap1)), 4 * B * ((gap1 - gap0) * 160 // 441 + 2 * up.H + (gap1 - gap0)), up),
    }
    print("resampler at B = %d, n = %d (44.1 kHz) <-> %d (16 kHz); median (best - worst) of %d calls" % (B, n, m, a.reps))
    result = {"tool": "wav_resample_rate", "streams": B, "samples": n, "low_samples": m, "reps": a.reps, "device": torch.cuda.get_device_name(0),
              "calls": {}}
    for name, (fn, need, rs) in calls.items():
        wall, stream = timed(fn, a.reps)
        us = lambda v: "%.1f (%.1f - %.1f)" % (statistics.median(v) * 1e6, min(v) * 1e6, max(v) * 1e6)
        rate = need / statistics.median(stream)
        print("  %-16s L %3d M %3d T %3d | wall %s us | stream %s us | moves %.3f MB: %.3f TB/s"
              % (name, rs.L, rs.M, rs.T, us(wall), us(stream), need / 1e6, rate / 1e12))
        result["calls"][name] = {"L": rs.L, "M": rs.M, "T": rs.T, "wall_us_median": round(statistics.median(wall) * 1e6, 2),
                                 "wall_us_min": round(min(wall) * 1e6, 2), "stream_us_median": round(statistics.median(stream) * 1e6, 2),
                                 "stream_us_min": round(min(stream) * 1e6, 2), "bytes_read_and_written": need,
                                 "bytes_per_second": round(rate, 1)}
    del hi, lo, back
    torch.cuda.empty_cache()
    copy, text = copy_rate()
    print("tools/probes/hbm_stream.py on this machine:")
    print("".join("    " + line + "\n" for line in text.splitlines()), end="")
    result["hbm_stream_copy_tb_per_s"] = copy
    if copy:
        for name, c in result["calls"].items():
            c["share_of_copy_rate"] = round(c["bytes_per_second"] / (copy * 1e12), 4)
            print("  %-16s %.3f TB/s = %.1f %% of the copy rate" % (name, c["bytes_per_second"] / 1e12, 100 * c["share_of_copy_rate"]))
    print(json.dumps(result, sort_keys=True))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(result, f, sort_keys=True, indent=1)


if __name__ == "__main__":
    main()
