#!/usr/bin/env python
"""Generate tests/golden/wav_io.npz from the REFERENCE's own `utils.audio.save_wav` (utils/audio.py:19-21; build container only).

The module is imported by the stand-in-module recipe of tools/make_preprocess_golden.py: `save_wav` calls numpy and scipy.io.wavfile only, so
empty stand-ins for lws and librosa make the import succeed, and tools/oracle_stubs supplies `Config` (its sample_rate, 16000, is what the
reference writes into the header).  Each clip is handed to `save_wav` as a COPY (the reference scales its argument in place) together with a
temporary path; the fixture records the clip, the sample rate and the bytes of the file.  Data only.

The clips, each a float32 array of at most 4096 samples:
    ordinary               seeded noise, peak about 0.3
    quiet                  peak < 0.01: the scale is 32767 / 0.01
    peak_f32_0p01          peak exactly float32(0.01), which is below the double 0.01: still the quiet branch
    peak_negative          the peak is at a negative sample
    peak_one               peak 1.0
    half_and_almost        peak 32767 / 65536, so the scale is exactly 65536: samples (k + 0.5) / 65536 and (k + 1 - 2^-8) / 65536 of both signs,
                           which truncation and rounding send to different integers
    over_32767             a peak p with fl32(p * fl32(32767 / p)) > 32767 (found by a seeded search): truncation brings it back
    zeros, length_1, tile_minus_1, tile_plus_1 (the peak in the last sample, so behind the last whole tile of VIAI_PCM_TILE)

Run:  python tools/make_wav_io_golden.py            (needs /root/reference)
"""
import os
import re
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(ROOT, "tools", "oracle_stubs"))
sys.path.insert(0, REF)
for name in ("lws", "librosa", "librosa.filters"):
    sys.modules.setdefault(name, types.ModuleType(name))

from utils import audio as RA          # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "wav_io.npz")
f32 = np.float32


def tile():
    text = open(os.path.join(ROOT, "include", "viai_hip.h")).read()
    return int(re.search(r"#define\s+VIAI_PCM_TILE\s+(\d+)", text).group(1))


def clips():
    rng = np.random.RandomState(20261020)
    noise = lambda n, a: (rng.uniform(-1, 1, n) * a).astype(f32)
    out = [("ordinary", noise(1000, 0.3)), ("quiet", noise(777, 0.005))]
    x = noise(500, 0.009)
    x[123] = f32(0.01)
    assert float(x[123]) < 0.01 and np.abs(x).max() == f32(0.01)
    out.append(("peak_f32_0p01", x))
    x = noise(640, 0.4)
    x[77] = f32(-0.7)
    out.append(("peak_negative", x))
    x = noise(512, 0.9)
    x[500] = f32(1.0)
    out.append(("peak_one", x))
    p = f32(32767) / f32(65536)
    assert f32(32767) / p == f32(65536)
    ks = np.array([0, 1, 2, 3, 100, 101, 4094, 4095, 16382, 16383, 32765], dtype=np.float64)
    half, almost = (ks + 0.5) / 65536, (ks + 1 - 2.0 ** -8) / 65536
    x = np.concatenate([[p], half, almost, -half, -almost]).astype(f32)
    assert np.array_equal(x.astype(np.float64)[1:], np.concatenate([half, almost, -half, -almost]))       # all exact in fp32
    out.append(("half_and_almost", x))
    for _ in range(100000):
        p = f32(rng.uniform(0.02, 1.0))
        if f32(p * (f32(32767) / p)) > f32(32767):
            break
    else:
        raise SystemExit("no peak whose scaled value exceeds 32767 was found")
    x = noise(300, float(p) * 0.9)
    x[0], x[299] = p, -p
    out.append(("over_32767", x))
    out.append(("zeros", np.zeros(100, dtype=f32)))
    out.append(("length_1", np.array([0.25], dtype=f32)))
    for name, n in (("tile_minus_1", tile() - 1), ("tile_plus_1", tile() + 1)):
        x = noise(n, 0.2)
        x[n - 1] = f32(-0.6)
        out.append((name, x))
    return out


def main():
    out = {"names": [], "rate": np.int64(RA.hparams.sample_rate)}
    with tempfile.TemporaryDirectory() as d:
        for name, x in clips():
            assert x.dtype == f32 and x.ndim == 1 and 1 <= x.size <= 4096
            path = os.path.join(d, name + ".wav")
            RA.save_wav(x.copy(), path)
            out["names"].append(name)
            out["clip." + name] = x
            out["file." + name] = np.frombuffer(open(path, "rb").read(), dtype=np.uint8)
    out["names"] = np.array(out["names"])
    np.savez_compressed(OUT, **out)
    print("wav_io -> %s (%.1f KB): %d clips at %d Hz" % (os.path.relpath(OUT, ROOT), os.path.getsize(OUT) / 1024, len(out["names"]), out["rate"]))


if __name__ == "__main__":
    main()
