#!/usr/bin/env python
"""Time per batch of the click detector (viai_amd.click_detect.find_clicks, csrc/click_detect.hip), what it detects, and the margin its CPU
test measures.

    times      B = 8 rows x 10 s at 16 kHz (160 000 samples a row, 40 tiles), the base signal of tests/click_detect_common.py with 12 clicks
               per 8969 samples: wall time of the whole Python call (checks, allocations, four launches, a synchronise) and stream time of the
               same call (events), median (best - worst), at order 32 (the default) and 128; next to `find_gaps` and `declick` on the same
               batch.  `find_gaps` is timed at THIS commit: its kernels are the parent's (their source moved into a shared header, their code
               did not change), so the figure stands for the parent's.  320 blocks are in flight, a block's time is its serial depth (`order`
               Burg stages of two barriers over 4096 samples): latencies of one batch, not a throughput claim.
    detection  seeds 0 to 5 of the base signal (test 4 of tests/test_click_detect_cpu.py): runs listed, clicks missed, stray runs, runs on
               the clean signal, and the SNR over the clicked samples against the clean signal before and after `declick_host`.
    margin     test 3: 4 x the largest relative difference of q / threshold between the restatement in the rule's summation order and the one
               with ordinary sums, over the judged samples of the case table.  Needs the built library, not a GPU.

    python tools/click_detect_rate.py [--reps 30] [--json profiles/click_detect_rate.json] [--host-only]

--host-only runs without a GPU and rewrites only the `detection` and `margin` keys of an existing file.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def margin():
    import click_detect_common as K
    m, seen = K.measured_margin()
    return {"margin": m, "judged_samples": seen,
            "what": "4 x max relative difference of q / threshold, rule order vs ordinary sums, over tests/click_detect_common.py"}


def detection():
    import numpy as np

    import click_detect_common as K
    from viai_amd.click_detect import declick_host, find_clicks_host
    out = []
    for seed in range(6):
        clean, hurt, pos, s = K.clicked(seed)
        g = find_clicks_host(hurt[None, :])
        rs = [(int(g.start[0, i]), int(g.length[0, i])) for i in range(int(g.count[0]))]
        missed = sum(not any(st <= c < st + ln for st, ln in rs) for c in pos)
        stray = sum(not any(c - 2 <= st and st + ln - 1 <= c + 32 + 2 for c in pos) for st, ln in rs)
        fixed = declick_host(hurt[None, :])[0][0]
        before, after = K.snr_db(clean, hurt, pos), K.snr_db(clean, fixed, pos)
        out.append({"seed": seed, "clicks": int(pos.size), "runs": len(rs), "missed": int(missed), "stray": int(stray),
                    "runs_on_clean": int(find_clicks_host(clean[None, :]).count[0]), "snr_db_before": round(float(before), 2),
                    "snr_db_after": round(float(after), 2), "snr_gain_db": round(float(after - before), 2)})
        print("seed %d: %s" % (seed, json.dumps(out[-1], sort_keys=True)))
    return out


def timed(fn, reps):
    """(wall seconds, stream seconds) per call, `reps` of each after three warm-up calls"""
    import torch
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
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "click_detect_rate.json"))
    ap.add_argument("--host-only", action="store_true")
    a = ap.parse_args()
    result = {}
    if a.host_only and os.path.exists(a.json):
        with open(a.json) as f:
            result = json.load(f)
    result["tool"] = "click_detect_rate"
    if not a.host_only:
        import numpy as np
        import torch
        if not torch.cuda.is_available():
            sys.exit("click_detect_rate: no GPU; a time is a measurement on the device or nothing (--host-only needs none)")
        import click_detect_common as K
        from viai_amd.click_detect import declick, find_clicks
        from viai_amd.gap_detect import find_gaps
        B, n = 8, 160000
        rows = []
        for b in range(B):
            parts = [K.clicked(6 * b + j)[1] for j in range(n // K.N_BASE + 1)]
            rows.append(np.concatenate(parts)[:n])
        wav = torch.from_numpy(np.stack(rows)).cuda()
        result.update({"rows": B, "samples_per_row": n, "sample_rate": 16000, "reps": a.reps, "device": torch.cuda.get_device_name(0),
                       "times": []})
        us = lambda v: "%.1f (%.1f - %.1f)" % (statistics.median(v) * 1e6, min(v) * 1e6, max(v) * 1e6)
        calls = [("find_gaps (this commit; the parent's kernels)", lambda: find_gaps(wav), None)]
        for order in (32, 128):
            calls.append(("find_clicks order %d" % order, lambda order=order: find_clicks(wav, order=order, max_gaps=512), order))
        calls.append(("declick order 32", lambda: declick(wav, max_gaps=512), 32))
        for label, fn, order in calls:
            got = fn()
            runs = int((got[1] if label.startswith("declick") else got).count.sum())
            wall, stream = timed(fn, a.reps)
            print("%-48s wall %s us | stream %s us | %d runs" % (label, us(wall), us(stream), runs))
            result["times"].append({"call": label, "order": order, "runs": runs, "wall_us_median": round(statistics.median(wall) * 1e6, 2),
                                    "wall_us_min": round(min(wall) * 1e6, 2), "stream_us_median": round(statistics.median(stream) * 1e6, 2),
                                    "stream_us_min": round(min(stream) * 1e6, 2),
                                    "seconds_of_audio_per_s": round(B * n / 16000.0 / statistics.median(stream), 1)})
    result["detection"] = detection()
    result["margin"] = margin()
    print(json.dumps(result, sort_keys=True))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(result, f, sort_keys=True, indent=1)


if __name__ == "__main__":
    main()
