#!/usr/bin/env python
"""Time per call and quality of the autoregressive gap fill (viai_amd.ar_fill.ar_fill, csrc/ar_fill.hip), and the tolerance its CPU test uses.

    times      B = 8 rows x 16 gaps each at L = 64, 160 and 1024 (order 32, context 1024): wall time of the whole Python call (checks, the
               clone, one launch, a synchronise) and stream time of the same call (events), median (best - worst).  128 blocks are in flight,
               one per gap; a block's time is its serial depth (32 Burg stages of two barriers, then L steps of a 32-term product), so the
               figures are latencies, not a throughput claim.  There is nothing at the parent commit to compare them with.
    baseline   the gap SNR (`viai_amd.metrics.wave_gap_stats` / `snr_db`, over the gap samples) of the AR fill on `synth.waveform` (three
               sinusoids plus uniform noise of amplitude 0.25) and on the same tones without the noise: the classical baseline beside which
               `AudioInpainter` can be reported.
    tolerance  max |host mirror - numpy restatement| / the row's peak over the case table of tests/ar_fill_common.py (`worst`) and ten times
               that (`allowed`): what tests/test_ar_fill_cpu.py asserts.  Needs the built library, not a GPU.

    python tools/ar_fill_rate.py [--reps 30] [--json profiles/ar_fill_rate.json] [--tolerance-only]

--tolerance-only runs without a GPU and rewrites only the `tolerance` key of an existing file.
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


def tolerance():
    import ar_fill_common as A
    from viai_amd.ar_fill import ar_fill_host
    worst = A.worst_relative_difference(ar_fill_host)
    return {"worst": worst, "allowed": 10.0 * worst, "cases": len(A.all_cases()),
            "what": "max |ar_fill_host - numpy fp64 restatement| / row peak over the filled samples of tests/ar_fill_common.py"}


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


def planted(B, K, L, n):
    """K gaps of L per row, evenly spaced with at least a context of 1024 clean samples between them"""
    import torch
    pitch = n // K
    assert pitch >= L + 1024
    start = torch.tensor([[k * pitch + 1024 + 3 * b for k in range(K)] for b in range(B)], dtype=torch.int32)
    return torch.full((B,), K, dtype=torch.int32), start, torch.full((B, K), L, dtype=torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "ar_fill_rate.json"))
    ap.add_argument("--tolerance-only", action="store_true")
    a = ap.parse_args()
    if a.tolerance_only:
        result = {}
        if os.path.exists(a.json):
            with open(a.json) as f:
                result = json.load(f)
        result.setdefault("tool", "ar_fill_rate")
        result["tolerance"] = tolerance()
        print(json.dumps(result["tolerance"], sort_keys=True))
        with open(a.json, "w") as f:
            json.dump(result, f, sort_keys=True, indent=1)
        return
    import torch
    if not torch.cuda.is_available():
        sys.exit("ar_fill_rate: no GPU; a time is a measurement on the device or nothing (--tolerance-only needs none)")
    from viai_amd import metrics, synth
    from viai_amd.ar_fill import ar_fill
    B, K, order, context = 8, 16, 32, 1024
    result = {"tool": "ar_fill_rate", "rows": B, "gaps_per_row": K, "order": order, "context": context, "reps": a.reps,
              "device": torch.cuda.get_device_name(0), "cases": [], "baseline": []}
    us = lambda v: "%.1f (%.1f - %.1f)" % (statistics.median(v) * 1e6, min(v) * 1e6, max(v) * 1e6)
    for L in (64, 160, 1024):
        n = K * (L + 1024 + 64)
        clean = synth.waveform(B, n, tag="ar.rate").cuda()
        gaps = tuple(g.cuda() for g in planted(B, K, L, n))
        hurt = clean.clone()
        for b in range(B):
            for k in range(K):
                s = int(gaps[1][b, k])
                hurt[b, s:s + L] = 0
        out, filled = ar_fill(hurt, gaps, order=order, context=context)
        assert int((filled == 1).sum()) == B * K
        wall, stream = timed(lambda: ar_fill(hurt, gaps, order=order, context=context), a.reps)
        copy_wall, copy_stream = timed(lambda: hurt.clone(), a.reps)
        print("L = %4d, n = %d: ar_fill wall %s us | stream %s us; the clone alone: stream %s us" % (L, n, us(wall), us(stream), us(copy_stream)))
        result["cases"].append({"gap": L, "samples": n, "wall_us_median": round(statistics.median(wall) * 1e6, 2),
                                "wall_us_min": round(min(wall) * 1e6, 2), "stream_us_median": round(statistics.median(stream) * 1e6, 2),
                                "stream_us_min": round(min(stream) * 1e6, 2),
                                "clone_stream_us_median": round(statistics.median(copy_stream) * 1e6, 2),
                                "filled_samples_per_s": round(B * K * L / statistics.median(stream), 1)})
        # the baseline figure: SNR over the gap samples, gap index by gap index, on the noisy clip and on its tones alone
        for label, ref in (("synth.waveform", clean), ("tones only", (clean - 0.25 * synth.uniform("ar.rate.n.r0", (B, n), -1, 1).cuda()))):
            damaged = ref.clone()
            damaged[hurt == 0] = 0
            est, _ = ar_fill(damaged, gaps, order=order, context=context)
            snr = torch.stack([metrics.snr_db(metrics.wave_gap_stats(ref, est, gaps[1][:, k], gaps[2][:, k])) for k in range(K)])
            entry = {"signal": label, "gap": L, "snr_db_median": round(float(snr.median()), 2), "snr_db_min": round(float(snr.min()), 2),
                     "snr_db_max": round(float(snr.max()), 2), "gaps": B * K}
            print("  %-15s gap SNR of the AR fill: median %.1f dB (%.1f - %.1f) over %d gaps" % (label, entry["snr_db_median"],
                                                                                               entry["snr_db_min"], entry["snr_db_max"], B * K))
            result["baseline"].append(entry)
    result["tolerance"] = tolerance()
    print(json.dumps(result, sort_keys=True))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(result, f, sort_keys=True, indent=1)


if __name__ == "__main__":
    main()
