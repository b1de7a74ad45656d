"""The shape of bench.py's contract line, without a GPU: the stdout line is a bounded projection of the detail record (round 5's 38 KB line
was not parsed by the driver)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _strings(o):
    if isinstance(o, str):
        yield o
    elif isinstance(o, dict):
        for k, v in o.items():
            yield k
            yield from _strings(v)
    elif isinstance(o, list):
        for v in o:
            yield from _strings(v)


def _load_bench():
    import importlib.util
    spec = importlib.util.spec_from_file_location("viai_bench", os.path.join(ROOT, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    argv, sys.argv = sys.argv, ["bench.py"]
    try:
        spec.loader.exec_module(b)
    finally:
        sys.argv = argv
    return b


def test_contract_line_projection_is_small_for_any_record():
    """compact_line on a worst-case record (every optional block present, long strings everywhere) stays under the limit"""
    b = _load_bench()
    long = "x" * 5000
    fams = {"family_number_%02d_f16x2" % i: 0.123 for i in range(40)}
    leg = {"value": 1.0, "unit": "clips/s", "ms_per_step": 1.0, "steps": 3, "config": {"workload": long}, "roofline": {"bound": "mfma", "frac": 0.5, "kernel": long, "note": long},
           "cpu_baseline": {"value": 1.0, "unit": "clips/s", "cores": 16, "kind": "port", "sample": long}}
    full = {"metric": b.METRIC, "value": 1.0, "unit": "clips/s", "n_gpus": 1, "steps": 1, "warmup": 1, "ms_per_step": 1.0, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f32", "data": "synthetic", "config": {"workload": long, "math": long, "launch": long, "note": long},
            "roofline": {"bound": "mfma", "achieved": 1.0, "peak": 2.0, "unit": "TFLOP/s", "frac": 0.5, "traffic": None, "kernel": long, "family": "f", "frac_by_kernel": fams,
                         "conv_time_share_by_kernel": fams, "kernels": {k: long for k in fams}, "peak_note": long, "step_floor": {"model": long, "largest_gaps": [long] * 10}},
            "stages": {"note": long, "large_batch": {"note": long}}, "extra": {"av": leg, "wavenet": leg, "audio_exact_fp32": leg, "failed": {"error": long}},
            "cpu_baseline": {"value": 1.0, "unit": "clips/s", "cores": 16, "kind": "port", "sample": long}}
    line = b.compact_line(full)
    assert len(line) < 8000 and max(len(s) for s in _strings(json.loads(line))) <= 120


def test_plain_run_is_the_default_and_full_is_an_option():
    b = _load_bench()
    argv = sys.argv
    try:
        sys.argv = ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"]
        a = b.parse()
        assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
        sys.argv = ["bench.py", "--full", "--dump-outputs", "out"]
        a = b.parse()
        assert a.full and a.dump_outputs == "out" and (a.steps, a.warmup) == (30, 5)
    finally:
        sys.argv = argv


def test_dump_outputs_stays_under_64_mb_with_a_fixed_sample(tmp_path):
    """float64 stays float64, the rest is float32; a set that would pass 64 MB keeps a seeded sample of each large array, the same every time"""
    import numpy as np
    import torch
    b = _load_bench()
    g = torch.Generator().manual_seed(0)
    arrays = {"small": torch.rand(3, 5, generator=g, dtype=torch.float64), "half": torch.rand(1000, generator=g).half(),
              "big": torch.rand(12_000_000, generator=g), "bigger": torch.rand(9_000_000, generator=g)}
    got = []
    for run in ("a", "b"):
        d = str(tmp_path / run)
        b.dump_outputs(d, arrays)
        assert sorted(os.listdir(d)) == ["big.npy", "bigger.npy", "half.npy", "small.npy"]
        assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= 64e6
        got.append({k: np.load(os.path.join(d, k + ".npy")) for k in arrays})
    x, y = got
    assert x["small"].dtype == np.float64 and np.array_equal(x["small"], arrays["small"].numpy())
    assert x["half"].dtype == np.float32 and np.array_equal(x["half"], arrays["half"].float().numpy())
    assert x["big"].dtype == np.float32 and x["big"].shape == (b.DUMP_SAMPLE,) and np.array_equal(x["big"], y["big"])
    assert np.isin(x["big"], arrays["big"].numpy()).all()
    # a set that fits is written whole
    d = str(tmp_path / "whole")
    b.dump_outputs(d, {"bigger": arrays["bigger"]})
    assert np.array_equal(np.load(os.path.join(d, "bigger.npy")), arrays["bigger"].numpy())
