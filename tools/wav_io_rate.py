#!/usr/bin/env python
"""Time per call of the PCM kernels (viai_amd.wav_io, csrc/wav_io.hip): decode, plain encode, normalised encode (S16 only) and patch with sparse
runs (a 1000-frame run about every 100 000 frames of every channel), for S16 x 1, S16 x 2, S24 x 2 and F32 x 2 at 2^20 and 2^24 frames.  Per
case: wall time of the whole Python call (checks, allocations, the launches, a synchronise), stream time of the same call (events), and the
bytes the call must move -- the sample bytes on one side plus the fp32 planes on the other -- per second of stream time.  Beside it, measured in
the same run:

    copy      `y.copy_(x)` of uint8 tensors with HALF that many bytes each, so the copy reads plus writes the same total.  The ceiling.
    torch     the obvious composition a user writes today: `view(int16).float() / 32768` and a transpose to planes; `clamp(round(x * 32768))` and
              a transpose back; three byte planes shifted and or-ed for S24; the peak, a scale and a truncating cast for the normalised encode.
              (Its clamp order and its normalised peak on the device differ in detail from the rule; it is a time, not a value, that is compared.)

patch moves only the runs' bytes: its line reports the time beside the clone of the data it always makes; no share is formed.
No threshold: the figures go into DESIGN.md 11.2p.

    python tools/wav_io_rate.py [--reps 30] [--json profiles/wav_io_rate.json]
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

BYTES = {"s16": 2, "s24": 3, "f32": 4}


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


def torch_decode(data, fmt, C):
    if fmt == "s16":
        x = data.view(torch.int16).float() / 32768
    elif fmt == "f32":
        x = data.view(torch.float32)
    else:
        b = data.view(-1, 3).to(torch.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        x = ((v ^ 0x800000) - 0x800000).float() / 8388608
    return x.view(-1, C).t().contiguous()


def torch_encode(wav, fmt):
    x = wav.t().contiguous().view(-1)
    if fmt == "f32":
        return x.view(torch.uint8)
    if fmt == "s16":
        return torch.clamp(torch.round(x * 32768), -32768, 32767).to(torch.int16).view(torch.uint8)
    q = torch.clamp(torch.round(x * 8388608), -8388608, 8388607).to(torch.int32)
    return torch.stack((q & 0xFF, (q >> 8) & 0xFF, (q >> 16) & 0xFF), 1).to(torch.uint8).view(-1)


def torch_encode_norm(wav):
    scale = 32767 / torch.clamp(wav.abs().max(), min=0.01)
    return (wav.t().contiguous().view(-1) * scale).to(torch.int16).view(torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "wav_io_rate.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("wav_io_rate: no GPU; a time is a measurement on the device or nothing")
    from viai_amd.gap_detect import Gaps
    from viai_amd.wav_io import decode_pcm, encode_pcm, patch_pcm
    result = {"tool": "wav_io_rate", "reps": a.reps, "device": torch.cuda.get_device_name(0), "cases": []}
    us = lambda v: "%.1f (%.1f - %.1f)" % (statistics.median(v) * 1e6, min(v) * 1e6, max(v) * 1e6)
    for frames in (1 << 20, 1 << 24):
        for fmt, C in (("s16", 1), ("s16", 2), ("s24", 2), ("f32", 2)):
            g = torch.Generator(device="cuda").manual_seed(frames % 1000 + C)
            wav = torch.rand(C, frames, generator=g, device="cuda") * 1.6 - 0.8
            data = encode_pcm(wav, fmt)
            moved = data.numel() + 4 * C * frames
            half = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
            other = torch.empty_like(half)
            K = (frames - 51000) // 100003 + 1
            start = torch.arange(K, dtype=torch.int32, device="cuda").mul(100003).add(50000).repeat(C, 1)
            gaps = Gaps(torch.full((C,), K, dtype=torch.int32, device="cuda"), start, torch.full_like(start, 1000))
            entry = {"frames": frames, "fmt": fmt, "channels": C, "bytes_moved": moved, "patch_runs": C * K}
            print("%s x %d, %d frames (%d bytes in plus out); median (best - worst) of %d calls" % (fmt, C, frames, moved, a.reps))
            calls = [("copy", lambda: other.copy_(half)), ("decode", lambda: decode_pcm(data, fmt, C)), ("torch_decode", lambda: torch_decode(data, fmt, C)),
                     ("encode", lambda: encode_pcm(wav, fmt)), ("torch_encode", lambda: torch_encode(wav, fmt))]
            if fmt == "s16":
                calls += [("encode_norm", lambda: encode_pcm(wav, fmt, normalize=True)), ("torch_encode_norm", lambda: torch_encode_norm(wav))]
            calls += [("patch", lambda: patch_pcm(data, wav, fmt, gaps)), ("clone", lambda: data.clone())]
            for name, fn in calls:
                wall, stream = timed(fn, a.reps)
                t = statistics.median(stream)
                entry[name] = {"wall_us_median": round(statistics.median(wall) * 1e6, 2), "wall_us_min": round(min(wall) * 1e6, 2),
                               "stream_us_median": round(t * 1e6, 2), "stream_us_min": round(min(stream) * 1e6, 2)}
                line = "  %-18s wall %s us | stream %s us" % (name, us(wall), us(stream))
                if name not in ("patch", "clone"):
                    entry[name]["gb_per_s"] = round(moved / t / 1e9, 2)
                    line += " | %.1f GB/s" % (moved / t / 1e9)
                print(line)
            for name in ("decode", "encode", "encode_norm"):
                if name in entry:
                    entry[name + "_share_of_copy_rate"] = round(entry["copy"]["stream_us_median"] / entry[name]["stream_us_median"], 4)
                    entry[name + "_times_the_torch_composition"] = round(entry["torch_" + name]["stream_us_median"] / entry[name]["stream_us_median"], 2)
                    print("  %s moves its bytes at %.1f %% of the copy's rate, %.1f x the torch composition"
                          % (name, 100 * entry[name + "_share_of_copy_rate"], entry[name + "_times_the_torch_composition"]))
            result["cases"].append(entry)
            del wav, data, half, other
            torch.cuda.empty_cache()
    print(json.dumps(result, sort_keys=True))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(result, f, sort_keys=True, indent=1)


if __name__ == "__main__":
    main()
