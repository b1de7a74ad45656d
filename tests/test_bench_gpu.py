"""bench.py's contract, run as the driver runs it (a subprocess, one JSON line on stdout)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

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


def run_bench(*argv, timeout=900, detail=False):
    """bench.py as the driver runs it.  The contract line must be the LAST line of stdout, strict JSON, < 8 KB, every string <= 120 characters
    (round 5's 38 KB line was not parsed by the driver); everything else bench.py measures goes to the --detail file."""
    import tempfile
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    with tempfile.TemporaryDirectory() as td:
        dpath = os.path.join(td, "detail.json")
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--detail", dpath] + list(argv), capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
        assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        lines = [l for l in r.stdout.splitlines() if l.startswith('{"metric"')]
        assert len(lines) == 1, r.stdout[-2000:]
        assert r.stdout.rstrip("\n").splitlines()[-1] == lines[0], "the contract line is not the last line of stdout"
        assert len(lines[0]) < 8192, len(lines[0])
        out = json.loads(lines[0], parse_constant=lambda c: (_ for _ in ()).throw(ValueError("non-strict JSON constant " + c)))
        assert max(len(s) for s in _strings(out)) <= 120
        for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"):
            assert k in out, k
        if detail:
            return out, json.load(open(dpath))
        return out


def test_gpus_2_spawns_its_own_ranks_and_exits_cleanly():
    """`python bench.py --gpus 2` with no launcher: bench.py re-runs itself as two ranks under torch.distributed.run; on this
    one-GPU box the ranks share cuda:0 and exchange over gloo (--share-gpu; RCCL refuses two ranks on one device), the bucketed exchange
    of the product step runs, rank 0 prints the one JSON line, and every rank leaves through destroy_process_group (exit status 0)."""
    out = run_bench("--full", "--gpus", "2", "--share-gpu", "--steps", "4", "--warmup", "2", "--batch", "2", "--bins", "128", "--frames", "64",
                    "--no-cpu-baseline")
    assert out["n_gpus"] == 2 and out["config"]["parallelism"] == "dp2" and out["config"]["global_batch"] == 4
    assert out["steps"] == 4 and out["warmup"] == 2 and out["scaling"] == "weak" and out["value"] > 0
    assert "comm_ms_exposed" in out["config"] and "ranks_share_devices" in out["config"]
    assert out["roofline"]["family"].endswith(("_f16x2", "_bf16x3", "_f32")) and 0 < out["roofline"]["frac"] < 1


def test_plain_run_times_the_steps_and_dumps_the_last_one(tmp_path):
    """a plain run (no --full) times exactly --steps steps and measures nothing else; --dump-outputs writes what the last timed step computed
    (the generated clips, the six loss scalars, both parameter arenas after the Adam updates), and the same arguments give the same files."""
    dumps = []
    for i in range(2):
        d = str(tmp_path / ("run%d" % i))
        out = run_bench("--steps", "3", "--warmup", "1", "--batch", "2", "--bins", "128", "--frames", "64", "--dump-outputs", d)
        assert out["steps"] == 3 and out["warmup"] == 1 and out["n_gpus"] == 1 and out["ms_per_step"] > 0
        assert abs(out["value"] - 2 * 1e3 / out["ms_per_step"]) < 0.01 * out["value"]
        for k in ("roofline", "stages", "extra", "cpu_baseline"):
            assert k not in out, k
        assert "launch_modes" not in out["config"] and "comm_ms_exposed" not in out["config"]
        assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= 64e6
        dumps.append({f[:-len(".npy")]: np.load(os.path.join(d, f)) for f in os.listdir(d)})
    a, b = dumps
    assert set(a) == {"fake", "losses", "params_G", "params_D"}
    assert a["fake"].shape == (2, 1, 128, 64) and a["fake"].dtype == np.float32
    assert a["losses"].shape == (6,) and a["losses"].dtype == np.float64
    assert a["params_G"].dtype == a["params_D"].dtype == np.float32 and a["params_G"].size > a["params_D"].size > 1000
    for k in a:
        assert np.isfinite(a[k]).all() and a[k].shape == b[k].shape, k
        assert np.allclose(a[k], b[k], rtol=1e-4, atol=1e-6), (k, float(np.abs(a[k] - b[k]).max()))


def test_gpus_n_without_devices_or_share_gpu_refuses():
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "64"], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode != 0 and "--share-gpu" in r.stderr


def test_kernel_families_come_from_the_library():
    """the roofline's kernel families are the names the library reports for each launch (viai_conv2d_last_kernel): one family per
    kernel instance the step runs, every family priced against the ceiling its suffix names; bench.py holds no dispatch mirror."""
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert "viai_conv2d_last_kernel" in src and "mirror of viai_" not in src
    line, out = run_bench("--full", "--steps", "3", "--warmup", "1", detail=True)
    # the contract line itself: roofline + cpu_baseline of the headline, and a few numbers of each bounded leg
    assert 0 < line["roofline"]["frac"] < 1 and line["roofline"]["bound"] == "mfma" and line["roofline"]["family"] == out["roofline"]["family"]
    assert line["roofline"]["avg_launch_us"] > 0 and line["roofline"]["peak"] > line["roofline"]["achieved"] > 0
    assert line["cpu_baseline"]["value"] > 0 and line["cpu_baseline"]["cores"] >= 1 and line["cpu_baseline"]["kind"] == "port"
    assert line["ms_per_step"] == out["ms_per_step"] and line["config"]["workload"].startswith("configs[1]")
    for k, unit in (("av", "clips/s"), ("wavenet", "samples/s"), ("audio_exact_fp32", "clips/s")):
        leg = line["extra"][k]
        assert "error" not in leg and leg["unit"] == unit and leg["value"] > 0 and 0 < leg["roofline"]["frac"] < 1, (k, leg)
    assert line["extra"]["av"]["cpu_baseline"]["value"] > 0 and line["extra"]["wavenet"]["cpu_baseline"]["value"] > 0
    assert line["roofline"].get("traffic") is None or line["roofline"]["traffic_source"].startswith("committed:")
    fams = out["roofline"]["conv_time_share_by_kernel"]
    assert "direct" in fams and "halo_wide256_f16x2" in fams and "wgrad_patch_f16x2" in fams and "unknown" not in fams
    assert abs(sum(fams.values()) - 1.0) < 0.02
    assert out["roofline"]["family"] in out["roofline"]["frac_by_kernel"]
    # the timed conv flops of the step are the SURVEY's 1 208 GFLOP (section 8d) to within the first-layer data gradients it leaves out
    assert abs(out["roofline"]["conv_gflop_per_step_timed"] - 1208.0) < 0.01 * 1208.0
    assert out["config"]["workload"].startswith("configs[1]") and out["n_gpus"] == 1 and "stages" in out
    # the live DVFS probe (round-4 advice: existence and finiteness only -- the ratio is a property of the SKU and the box, not of the code)
    pl = out["roofline"]["power_limit"]
    assert pl["ratio"] > 0 and pl["random_operand_us"] > 0 and pl["ratio"] == pl["ratio"]
    # round 5: the whole-step floor (per-launch max(flops / sustained ceiling, bytes / copy bandwidth) over a single-stream step), the counter-derived
    # MFMA-busy figures, and the bounded legs on the other configs / the exact-fp32 mode
    rf = out["roofline"]
    sf = rf["step_floor"]
    assert 0 < rf["step_floor_ms"] == sf["step_floor_ms"] < out["ms_per_step"] and 0 < rf["frac_of_floor"] < 1
    assert abs(sf["floor_ms_by_bound"]["mfma"] + sf["floor_ms_by_bound"]["hbm"] - sf["step_floor_ms"]) < 0.01 and sf["single_stream_ms"] > sf["step_floor_ms"]
    assert len(sf["largest_gaps"]) == 10 and all(g["measured_us"] > 0 for g in sf["largest_gaps"]) and sf["launches_per_step"] > 100
    assert sf["family_bound"]["halo_c32_f16x2"]["bound"] == "hbm" and sf["family_bound"]["halo_wide256_f16x2"]["bound"] == "mfma"
    mb = rf["mfma_busy"]
    assert 0 < mb["whole_step"] < mb["conv_kernels_time_weighted"] < 1 and mb["source"].startswith("committed: profiles/")
    assert sf["step_floor_at_peak_ms"] < sf["step_floor_ms"] and 0 < sf["frac_of_floor_at_peak"] < sf["frac_of_floor"]
    ex = out["extra"]
    assert set(ex) == {"av", "wavenet", "audio_exact_fp32"}
    for k, unit in (("av", "clips/s"), ("wavenet", "samples/s"), ("audio_exact_fp32", "clips/s")):
        assert "error" not in ex[k] and ex[k]["unit"] == unit and ex[k]["value"] > 0 and "roofline" in ex[k], (k, ex[k].get("error"))
    assert ex["audio_exact_fp32"]["ms_per_step"] > out["ms_per_step"] and ex["av"]["config"]["workload"].startswith("configs[2]")


@pytest.mark.parametrize("config", ["av", "av_msd"])
def test_vision_infused_configs_print_roofline_and_cpu_baseline(config):
    out = run_bench("--full", "--config", config, "--steps", "2", "--warmup", "1", "--batch", "1", "--bins", "256", "--frames", "32")
    assert out["config"]["workload"].startswith("configs[%d]" % (2 if config == "av" else 3))
    rf = out["roofline"]
    assert rf["bound"] == "mfma" and 0 < rf["frac"] < 1 and rf["family"] in rf["frac_by_kernel"]
    assert out["cpu_baseline"]["kind"] == "port" and out["cpu_baseline"]["value"] > 0 and out["cpu_baseline"]["unit"] == "clips/s"
    assert out["config"]["algorithmic_gflop_per_step"] > 0


def test_wavenet_config_prints_the_synthesis_line():
    out = run_bench("--full", "--config", "wavenet", "--steps", "192", "--warmup", "64")
    assert out["unit"] == "samples/s" and out["steps"] == 192 and out["value"] > 1000
    rf = out["roofline"]
    assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and 0 < rf["frac"] < 1 and 90e6 < rf["algorithmic_bytes_per_step"] < 110e6
    assert out["cpu_baseline"]["unit"] == "samples/s" and 0 < out["cpu_baseline"]["value"] < out["value"]
