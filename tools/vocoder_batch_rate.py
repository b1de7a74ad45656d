#!/usr/bin/env python
"""Rate of the WaveNet batch assembly (viai_amd.vocoder_batch): `--rows` pairs of eight-second utterances cropped to the upstream-sized
`max_time_steps` (8000 samples: 31 frames of 256), in class form (y, classes, c) and with the dense one-hot input on top, as wall time of the whole
call (plan, table upload, allocation, one launch), as stream time of the same call (events), and as GB/s written by it.  Beside it the host route on the
same box: the same batch assembled in numpy the way `collate_fn` does it (crop, pad, one-hot by an identity-matrix gather, transposes) plus the copy
of the results to the device.  No threshold: the figures go into DESIGN.md 11.2j.

    python tools/vocoder_batch_rate.py [--rows 8] [--seconds 8] [--max-time-steps 8000] [--reps 20]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed_all(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def device_time(fn, reps):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        ev0.record()
        fn()
        ev1.record()
        torch.cuda.synchronize()
        out.append(ev0.elapsed_time(ev1) * 1e-3)
    return out


def host_collate(rows, starts, frames, hop, K, one_hot):
    """the batch in numpy, then on the device: what a host loader and its .cuda() calls do"""
    B, L = len(rows), max(frames)
    T = L * hop
    y = np.zeros((B, T), dtype=np.int64)
    c = np.zeros((B, L, rows[0][1].shape[1]), dtype=np.float32)
    for b, ((s, m), st, f) in enumerate(zip(rows, starts, frames)):
        y[b, :f * hop] = s[st * hop:(st + f) * hop]
        c[b, :f] = m[st:st + f]
    out = [torch.from_numpy(y[:, :, None]).cuda(), torch.from_numpy(np.ascontiguousarray(c.transpose(0, 2, 1))).cuda(),
           torch.tensor([f * hop for f in frames]).cuda()]
    if one_hot:
        x = np.zeros((B, T, K), dtype=np.float32)
        for b, f in enumerate(frames):
            x[b, :f * hop] = np.eye(K, dtype=np.float32)[y[b, :f * hop]]
        out.append(torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1))).cuda())
    else:
        out.append(torch.from_numpy(y.astype(np.int32)).cuda())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=8.0)
    ap.add_argument("--max-time-steps", type=int, default=8000)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    from viai_amd.audio import AudioConfig
    from viai_amd.vocoder_batch import VocoderBatcher, crop_plan
    hop, D, K = AudioConfig.hop_size, AudioConfig.num_mels, 256
    rng = np.random.RandomState(0)
    n = [int(a.seconds * AudioConfig.sample_rate) // hop + i for i in range(a.rows)]                    # rows of different lengths, all cropped
    host = [(rng.randint(0, K, f * hop).astype(np.int32), rng.standard_normal((f, D)).astype(np.float32)) for f in n]
    dev = [(torch.from_numpy(s).cuda(), torch.from_numpy(m).cuda()) for s, m in host]
    starts, frames = crop_plan(n, hop, a.max_time_steps, rng=np.random.RandomState(1))
    B, L = a.rows, max(frames)
    T = L * hop
    print("batch: %d rows of %d to %d frames cropped to %d (T = %d), hop %d, D %d, K %d; best - worst of %d calls"
          % (B, min(n), max(n), L, T, hop, D, K, a.reps))
    span = lambda v, unit=1e3: "%.3f - %.3f" % (min(v) * unit, max(v) * unit)
    for name, one_hot in (("class form (y, classes, c)", False), ("with the one-hot x", True)):
        vb = VocoderBatcher(max_time_steps=a.max_time_steps, one_hot=one_hot)
        call = lambda: vb(dev, starts=starts)
        batch = call()
        written = sum(t.numel() * t.element_size() for t in (batch.y, batch.classes, batch.c, batch.x) if t is not None)
        wall, stream = timed_all(call, a.reps), device_time(call, a.reps)
        t_host = timed_all(lambda: host_collate(host, starts, frames, hop, K, one_hot), max(3, a.reps // 4))
        ref = host_collate(host, starts, frames, hop, K, one_hot)
        same = torch.equal(ref[0], batch.y) and torch.equal(ref[1], batch.c) and torch.equal(ref[3], batch.x if one_hot else batch.classes)
        print("%s: %.2f MB written" % (name, written / 1e6))
        print("  device route, whole call: wall %s ms | stream time %s ms = %.1f GB/s written at the best stream time (%.1f at the best wall time)"
              % (span(wall), span(stream), written / min(stream) / 1e9, written / min(wall) / 1e9))
        print("  host route, numpy assembly + copies to the device: %s ms; results %s the device route's" % (span(t_host), "equal" if same else "DIFFER from"))


if __name__ == "__main__":
    main()
