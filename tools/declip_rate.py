#!/usr/bin/env python
"""Quality and time per sweep of the bound-constrained Janssen restoration (viai_amd.declip.declip_fill, csrc/declip.hip) and the tolerance
its CPU test uses.

    tolerance  max |declip_fill_host (fp32) - numpy restatement before its rounding (fp64)| / the row's peak over the solved samples of the
               speech-like rows and the case table of tests/declip_common.py: `measured`, and ten times that (`allowed`), which is what
               tests/test_declip_cpu.py asserts.  Host only.
    quality    SNR in dB over the clipped samples (the listed samples inside [256, n - 256); the lists also hold the unclipped peaks of the head
               and tail) of `declip_common.speechlike(seed)` (seeds 1 and 2, clipped at 0.3 of the peak) from the host
               mirrors, which give the device's bits: the clipped signal itself, `janssen_fill_host(order=32, context=256, iters=3)` on the same
               lists, the unconstrained wide-window solve (rounds=0, sweeps=1), and `declip_fill_host` at its defaults for sweeps 1 to 4; with
               each, how many listed samples lie inside the clipping level.  Host only.
    times      stream time (events) per sweep of `declip_fill` at its defaults (one launch; measured as (sweeps=3 minus sweeps=1) / 2 so that
               the clones are not counted) for 1, 8 and 64 rows of 1 s at 16 kHz, every row a speech-like signal clipped at 0.3 with
               max_gaps=1024.  Median of --reps after three warm-up calls.  A block's time is its serial depth (per iteration p Burg stages,
               then up to 1 + rounds solves of M columns of two barriers and M back-substitution steps), so the figures are latencies of the
               busiest cluster, not a throughput claim.  Bank conflicts and occupancy are NOT measured.  Needs the GPU; without one `times`
               says "not measured".

    python tools/declip_rate.py [--reps 20] [--json profiles/declip_rate.json] [--host-only]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SWEEPS = (1, 2, 3, 4)


def tolerance():
    import declip_common as D
    from viai_amd.declip import declip_fill_host
    worst = D.worst_relative_difference(declip_fill_host)
    return {"measured": worst, "allowed": 10.0 * worst, "inputs": len(D.tolerance_inputs()),
            "what": "max |declip_fill_host (fp32) - numpy fp64 restatement (np.dot, dense G, np.linalg.solve) before its rounding to fp32| / row "
                    "peak over the solved samples of tests/declip_common.py (speech-like seeds 1 and 2 at 1 and 3 sweeps, and the case table); "
                    "half an fp32 unit of the peak is 3e-8"}


def quality():
    import declip_common as D
    from viai_amd.declip import declip_fill_host
    from viai_amd.janssen import janssen_fill_host
    out = []
    for seed in D.SEEDS:
        c = D.speech_case(seed)
        wav, gaps, clean = c["wav"], c["gaps"], c["clean"]
        m = D.clipped_mask(c)
        rec = {"signal": "speechlike(seed=%d), clipped at %.1f" % (seed, D.CLIP), "runs": int(gaps[0][0]),
               "listed_samples": int(D.listed_mask(gaps, wav.shape).sum()), "clipped_samples": int(m.sum()),
               "clipped_snr_db": round(D.snr_db(clean, wav, m), 2)}
        jn, _ = janssen_fill_host(wav, gaps, order=32, context=256, iters=3)
        rec["janssen_fill_snr_db"] = round(D.snr_db(clean, jn, m), 2)
        rec["janssen_fill_inside_level"] = D.violations(wav, jn, m)
        un, _ = declip_fill_host(wav, gaps, rounds=0, sweeps=1)
        rec["unconstrained_wide_window_snr_db"] = round(D.snr_db(clean, un, m), 2)
        rec["unconstrained_wide_window_inside_level"] = D.violations(wav, un, m)
        for s in SWEEPS:
            got, _ = declip_fill_host(wav, gaps, sweeps=s)
            rec["declip_snr_db_sweeps%d" % s] = round(D.snr_db(clean, got, m), 2)
            rec["declip_inside_level_sweeps%d" % s] = D.violations(wav, got, m)
        out.append(rec)
    return out


def stream_us(fn, reps):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(reps):
        ev0.record()
        fn()
        ev1.record()
        torch.cuda.synchronize()
        ts.append(ev0.elapsed_time(ev1) * 1e3)
    return {"median": round(statistics.median(ts), 2), "min": round(min(ts), 2), "max": round(max(ts), 2)}


def times(reps):
    import numpy as np
    import torch

    import declip_common as D
    from viai_amd.declip import declip_fill
    from viai_amd.gap_detect import find_gaps
    out = []
    rows = np.stack([D.speechlike(100 + b, n=16000)[1] for b in range(64)])
    for B in (1, 8, 64):
        wav = torch.from_numpy(rows[:B]).cuda()
        gaps = find_gaps(wav, clip=D.CLIP, min_len=1, max_gaps=1024)
        one = stream_us(lambda: declip_fill(wav, gaps, sweeps=1), reps)
        three = stream_us(lambda: declip_fill(wav, gaps, sweeps=3), reps)
        rec = {"rows": B, "samples_per_row": 16000, "runs_per_row_max": int(gaps.count.max()), "call_us_sweeps1": one, "call_us_sweeps3": three,
               "us_per_sweep": round((three["median"] - one["median"]) / 2.0, 2)}
        out.append(rec)
        print(json.dumps(rec), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "declip_rate.json"))
    ap.add_argument("--host-only", action="store_true")
    args = ap.parse_args()
    res = {"tolerance": tolerance(), "quality": quality(),
           "defaults": "order=32, context=256, iters=2, rounds=3, sweeps=3: choices from a numpy prototype, not tuned on the device",
           "not_measured": ["LDS bank conflicts", "occupancy", "a throughput with every CU busy"]}
    if args.host_only:
        res["times"] = "not measured: no GPU run"
    else:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("declip_rate: no GPU; --host-only writes the tolerance and quality entries alone")
        res["times"] = {"reps": args.reps, "what": "stream time per Python call, microseconds; us_per_sweep = (sweeps=3 - sweeps=1) / 2",
                        "cases": times(args.reps)}
    with open(args.json, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res["tolerance"]))
    print(json.dumps(res["quality"]))


if __name__ == "__main__":
    main()
