#!/usr/bin/env python
"""Time per call of gap detection (viai_amd.gap_detect.find_gaps, csrc/gap_detect.hip) at B = 8 clips of n = 2^20 and 2^24 samples, at three damage
densities: none, sparse (a 1000-sample dropout about every 100 000 samples) and half (every sample zero with probability 1/2: runs at every scale,
about n / 4 of them per row).  Per case: wall time of the whole Python call (checks, the allocations, three launches, a synchronise), stream time
of the same call (events), and the waveform bytes 4 B n -- every sample is read once -- per second of stream time.  Beside it, on the same
machine and the same tensor:

    copy      `y.copy_(x)`: reads the same bytes (and writes as many).  Its read rate is the ceiling for a pass that must read every sample.
    torch     what a user writes today without the kernel: isfinite / abs / compare, a diff of the padded mask, two `nonzero` (which synchronise
              and whose size depends on the data), a length filter.  No merging, so it does less than find_gaps.  The baseline.

No threshold: the figures go into DESIGN.md 11.2m.

    python tools/gap_detect_rate.py [--streams 8] [--reps 30] [--json profiles/gap_detect_rate.json]
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


def torch_gaps(wav, min_len):
    """(row, start, length) of the kept raw runs, out of torch ops"""
    bad = (~torch.isfinite(wav)) | (wav.abs() <= 0)
    edge = torch.diff(torch.nn.functional.pad(bad.to(torch.int8), (1, 1)), dim=1)
    s, e = (edge == 1).nonzero(), (edge == -1).nonzero()
    keep = (e[:, 1] - s[:, 1]) >= min_len
    return s[keep, 0], s[keep, 1], (e[:, 1] - s[:, 1])[keep]


def clip(B, n, density, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    wav = torch.rand(B, n, generator=g, device="cuda") * 0.8 + 0.1
    if density == "sparse":
        for b in range(B):
            for s in range(50000 + 7 * b, n - 1000, 100003):
                wav[b, s:s + 1000] = 0
    elif density == "half":
        wav[torch.rand(B, n, generator=g, device="cuda") < 0.5] = 0
    return wav


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=8)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "gap_detect_rate.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gap_detect_rate: no GPU; a time is a measurement on the device or nothing")
    from viai_amd.gap_detect import find_gaps
    B = a.streams
    result = {"tool": "gap_detect_rate", "streams": B, "reps": a.reps, "device": torch.cuda.get_device_name(0), "cases": []}
    us = lambda v: "%.1f (%.1f - %.1f)" % (statistics.median(v) * 1e6, min(v) * 1e6, max(v) * 1e6)
    for n in (1 << 20, 1 << 24):
        for density in ("none", "sparse", "half"):
            wav = clip(B, n, density, n % 1000 + len(density))
            other = torch.empty_like(wav)
            need = 4 * B * n
            # sparse: min_len 64, the default; half: min_len 1, every run is kept (the most the emit launch can be asked to do)
            min_len = 1 if density == "half" else 64
            runs = int(find_gaps(wav, min_len=min_len).count.sum())
            entry = {"samples": n, "density": density, "min_len": min_len, "runs": runs, "waveform_bytes": need}
            print("B = %d, n = %d, %s damage (min_len %d): %d runs; median (best - worst) of %d calls" % (B, n, density, min_len, runs, a.reps))
            for name, fn in (("find_gaps", lambda: find_gaps(wav, min_len=min_len)), ("copy", lambda: other.copy_(wav)),
                             ("torch", lambda: torch_gaps(wav, min_len))):
                wall, stream = timed(fn, a.reps if name != "torch" else max(3, a.reps // 5))
                t = statistics.median(stream if name != "torch" else wall)            # the torch composition synchronises inside itself
                print("  %-10s wall %s us | stream %s us | %.1f GB/s of waveform read" % (name, us(wall), us(stream), need / t / 1e9))
                entry[name] = {"wall_us_median": round(statistics.median(wall) * 1e6, 2), "wall_us_min": round(min(wall) * 1e6, 2),
                               "stream_us_median": round(statistics.median(stream) * 1e6, 2), "stream_us_min": round(min(stream) * 1e6, 2),
                               "waveform_gb_per_s": round(need / t / 1e9, 2)}
            entry["share_of_copy_rate"] = round(entry["find_gaps"]["waveform_gb_per_s"] / entry["copy"]["waveform_gb_per_s"], 4)
            entry["times_the_torch_composition"] = round(entry["find_gaps"]["waveform_gb_per_s"] / entry["torch"]["waveform_gb_per_s"], 2)
            print("  find_gaps reads at %.1f %% of the copy's rate, %.1f x the torch composition"
                  % (100 * entry["share_of_copy_rate"], entry["times_the_torch_composition"]))
            result["cases"].append(entry)
            del wav, other
            torch.cuda.empty_cache()
    print(json.dumps(result, sort_keys=True))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(result, f, sort_keys=True, indent=1)


if __name__ == "__main__":
    main()
