#!/usr/bin/env python
"""Time per call and quality of Janssen's AR interpolation (viai_amd.janssen.janssen_fill, csrc/janssen_fill.hip) beside the Burg cross-fade
(`ar_fill`) on the same lists, and the tolerances its CPU test uses.

    tolerance  max |janssen_fill_host - numpy restatement| / the row's peak over the solved samples of the case table of
               tests/janssen_common.py: `measured` over the sigma = 0.01 cases and ten times that (`allowed`), and the same pair for the
               noiseless row (`noiseless_measured`, `noiseless_allowed`): what tests/test_janssen_cpu.py asserts.  Host only.
    quality    gap SNR in dB of both methods from the host mirrors on the rows of the issue's table (`jn.crackle` three rows, `jn.single` four
               gaps; n = 4200, sigma 0.01, order 32, context 1024) at iters 1, 3 and 8.  Host only.
    times      stream time (events) per call of `janssen_fill` at iters 1, 3 and 8 and of `ar_fill` on the same lists: the three crackle rows
               as one batch, and single gaps of 16, 64 and 240.  Median of --reps after three warm-up calls.  A block's time is its serial
               depth (p Burg stages, M columns of two barriers, M back-substitution steps, per iteration), so the figures are latencies of
               one to three busy blocks, not a throughput claim.  Bank conflicts and occupancy are NOT measured.  Needs the GPU; without one
               `times` says "not measured".

    python tools/janssen_rate.py [--reps 30] [--json profiles/janssen_fill_rate.json] [--host-only]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ITERS = (1, 3, 8)


def tolerance():
    import janssen_common as J
    from viai_amd.janssen import janssen_fill_host
    noisy, clean = J.worst_relative_difference(janssen_fill_host, False), J.worst_relative_difference(janssen_fill_host, True)
    return {"measured": noisy, "allowed": 10.0 * noisy, "noiseless_measured": clean, "noiseless_allowed": 10.0 * clean,
            "cases": len(J.all_cases()),
            "what": "max |janssen_fill_host - numpy fp64 restatement (np.dot, dense G, np.linalg.solve)| / row peak over the solved samples of "
                    "tests/janssen_common.py, after both were rounded to fp32 once; 0.0 means every fp32 bit agreed"}


def quality_sets():
    import ar_fill_common as A
    import janssen_common as J
    return (("jn.crackle", J.crackle_clean(), J.CRACKLE_ROWS, 64), ("jn.single", J.single_clean(), J.SINGLE_ROWS, 1)), A, J


def quality():
    from viai_amd.ar_fill import ar_fill_host
    from viai_amd.janssen import janssen_fill_host
    sets, A, J = quality_sets()
    rows_out = []
    for tag, clean, rows, K in sets:
        hurt, gaps = A.damage(clean, rows), A.lists(rows, K)
        burg, _ = ar_fill_host(hurt, gaps, order=32, context=1024)
        jn = {it: janssen_fill_host(hurt, gaps, order=32, context=1024, iters=it)[0] for it in ITERS}
        for b, r in enumerate(rows):
            sp = J.spans(r)
            rec = {"signal": tag, "row": b, "runs": len(r), "run_length": r[0][1], "sigma": 0.01,
                   "burg_snr_db": round(A.gap_snr_db(clean[b], burg[b], sp), 2)}
            for it in ITERS:
                rec["janssen_snr_db_iters%d" % it] = round(A.gap_snr_db(clean[b], jn[it][b], sp), 2)
            rows_out.append(rec)
    return rows_out


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
    import torch
    from viai_amd.ar_fill import ar_fill
    from viai_amd.janssen import janssen_fill
    sets, A, J = quality_sets()
    work = [("crackle: 3 rows, 40 x 3, 60 x 2 and 30 x 5 samples", A.damage(sets[0][1], sets[0][2]), A.lists(sets[0][2], 64))]
    for L in (16, 64, 240):
        rows = [[(2000, L)]]
        work.append(("one gap of %d" % L, A.damage(sets[1][1][:1], rows), A.lists(rows, 1)))
    out = []
    for name, hurt, gaps in work:
        wav = torch.from_numpy(hurt).cuda()
        g = tuple(torch.from_numpy(x).cuda() for x in gaps)
        rec = {"lists": name, "rows": int(wav.size(0)), "K": int(g[1].size(1)),
               "ar_fill_stream_us": stream_us(lambda: ar_fill(wav, g, order=32, context=1024), reps)}
        for it in ITERS:
            rec["janssen_fill_stream_us_iters%d" % it] = stream_us(lambda: janssen_fill(wav, g, order=32, context=1024, iters=it), reps)
        out.append(rec)
        print(json.dumps(rec), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "janssen_fill_rate.json"))
    ap.add_argument("--host-only", action="store_true")
    args = ap.parse_args()
    res = {"tolerance": tolerance(), "quality": quality(),
           "not_measured": ["LDS bank conflicts", "occupancy", "a throughput with many busy clusters per launch"]}
    if args.host_only:
        res["times"] = "not measured: no GPU run"
    else:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("janssen_rate: no GPU; --host-only writes the tolerance and quality entries alone")
        res["times"] = {"reps": args.reps, "what": "stream time per Python call (the clone and one launch), microseconds", "cases": times(args.reps)}
    with open(args.json, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res["tolerance"]))


if __name__ == "__main__":
    main()
