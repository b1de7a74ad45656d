"""`viai_dropout` as a streaming kernel, next to `viai_add_scale` on the same buffers: n = 8 * 8192 * 512 floats (the residual tensor of the
reference-width WaveNet at B = 8, T = 8192), p = 0.05.

Four kernels alternating in one process, HIP events around `INNER` launches, warm-up, median of `--reps` repetitions:
  dropout, dropout in place (8 B per element), add_scale(a, NULL) (8 B: the like-for-like comparison), add_scale(a, b) (12 B).
Two modes: `same` reuses one buffer set (268 MB touched: partly served by the 256 MiB cache), `rot` takes 8 buffer sets in turn (HBM).
GB/s = bytes the algorithm moves / time.

    python tools/wn_dropout_rate.py [--out profiles/wn_dropout_rate.json] [--reps 25]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from viai_amd import _lib  # noqa: E402

INNER, SETS = 16, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wn_dropout_rate.json"))
    ap.add_argument("--reps", type=int, default=25)
    args = ap.parse_args()
    lib = _lib.load()
    n = 8 * 8192 * 512
    xs = [torch.randn(n, device="cuda") for _ in range(SETS)]
    bs = [torch.randn(n, device="cuda") for _ in range(SETS)]
    ys = [torch.empty(n, device="cuda") for _ in range(SETS)]
    st = torch.cuda.current_stream().cuda_stream
    r5 = 0.5 ** 0.5
    kernels = {
        "dropout": (8, lambda i: lib.viai_dropout(xs[i].data_ptr(), ys[i].data_ptr(), n, 0.05, 1234, 7, st)),
        "dropout_inplace": (8, lambda i: lib.viai_dropout(ys[i].data_ptr(), ys[i].data_ptr(), n, 0.05, 1234, 7, st)),
        "add_scale_nob": (8, lambda i: lib.viai_add_scale(xs[i].data_ptr(), 0, ys[i].data_ptr(), r5, n, st)),
        "add_scale_b": (12, lambda i: lib.viai_add_scale(xs[i].data_ptr(), bs[i].data_ptr(), ys[i].data_ptr(), r5, n, st)),
    }

    def timed(fn, rot):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(INNER):
            _lib.check(fn(i % SETS if rot else 0), "launch")
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / INNER

    doc = {"n": n, "p": 0.05, "launches_per_timing": INNER, "reps": args.reps, "device": torch.cuda.get_device_name(0)}
    for mode, rot in (("same", False), ("rot", True)):
        for _, fn in kernels.values():
            for _ in range(3):
                timed(fn, rot)
        ms = {k: [] for k in kernels}
        for _ in range(args.reps):
            for k, (_, fn) in kernels.items():
                ms[k].append(timed(fn, rot))
        doc[mode] = {k: {"bytes_per_element": kernels[k][0], "ms": statistics.median(v), "ms_min_max": [min(v), max(v)],
                         "GBps": kernels[k][0] * n / statistics.median(v) / 1e6} for k, v in ms.items()}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({m: {k: round(v["GBps"]) for k, v in doc[m].items()} for m in ("same", "rot")}))


if __name__ == "__main__":
    main()
