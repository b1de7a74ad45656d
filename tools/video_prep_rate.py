#!/usr/bin/env python
"""Time of the three passes of the video front end (viai_amd.video, csrc/video_prep.hip) on one clip of 180 frames of 480 x 640: the motion pass
over both flow stacks, the box pass over the tile flags, and the prepare pass (crop + pad + resize + flip + crop + normalise) for the image and
for the flow pair, in the train form (256 -> window of 224, flipped) and the eval form (straight to 224).

Per pass: stream time from device events (median, best and worst of `--reps` calls after warm-up calls), the bytes the pass must move by the
model of DESIGN.md 11.2n, those bytes per second, and beside it the rate of a torch device copy that moves the same number of bytes (half read,
half written), timed the same way in the same process.  The spread between the best and the worst call is written down with every median; the
spread from machine to machine is not something one run can know.

The motion and box passes are timed at the C entry points with a workspace made once; the prepare passes are whole `viai_amd.video.prepare`
calls (two allocations, the table launch and the resampling launch), so their times hold host and launch overhead too.

No rate here is a threshold: the figures go into DESIGN.md 11.2n so that a later change has something to beat.

    python tools/video_prep_rate.py [--frames 180] [--reps 30] [--json profiles/video_prep_rate.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps, warm=5):
    """stream seconds per call"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t = []
    for _ in range(reps):
        ev0.record()
        fn()
        ev1.record()
        torch.cuda.synchronize()
        t.append(ev0.elapsed_time(ev1) * 1e-3)
    return t


def copy_rate(nbytes, reps):
    """a device copy that moves nbytes in all: nbytes / 2 read and nbytes / 2 written"""
    half = max(int(nbytes) // 2, 16)
    src = torch.empty(half, dtype=torch.uint8, device="cuda").fill_(3)
    dst = torch.empty_like(src)
    t = timed(lambda: dst.copy_(src), reps)
    return 2 * half, t


def entry(name, t, nbytes, copy_bytes, copy_t, extra=None):
    med, cmed = statistics.median(t), statistics.median(copy_t)
    e = {"pass": name, "us_median": round(med * 1e6, 2), "us_min": round(min(t) * 1e6, 2), "us_max": round(max(t) * 1e6, 2),
         "bytes_moved": int(nbytes), "gb_per_s": round(nbytes / med / 1e9, 2),
         "copy_us_median": round(cmed * 1e6, 2), "copy_us_min": round(min(copy_t) * 1e6, 2), "copy_us_max": round(max(copy_t) * 1e6, 2),
         "copy_gb_per_s": round(copy_bytes / cmed / 1e9, 2)}
    e["share_of_copy_rate"] = round(e["gb_per_s"] / e["copy_gb_per_s"], 4)
    e.update(extra or {})
    print("  %-28s %9.1f us (%.1f - %.1f) | %11d bytes | %8.1f GB/s | copy of as many bytes %8.1f GB/s | %.2f of it"
          % (name, e["us_median"], e["us_min"], e["us_max"], nbytes, e["gb_per_s"], e["copy_gb_per_s"], e["share_of_copy_rate"]))
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=180)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "video_prep_rate.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("video_prep_rate: no GPU; a time is a measurement on the device or nothing")
    from viai_amd import _lib
    from viai_amd.ops import _stream
    from viai_amd.video import motion_box, prepare
    lib = _lib.load()
    N, H, W = a.frames, a.height, a.width
    g = torch.Generator(device="cuda").manual_seed(11)
    image = torch.randint(0, 256, (N, H, W, 3), generator=g, device="cuda", dtype=torch.uint8)
    fx = torch.randint(126, 129, (N, H, W), generator=g, device="cuda", dtype=torch.uint8)       # quiet: |v - 127| <= 1 never enters the mask
    fy = torch.randint(126, 129, (N, H, W), generator=g, device="cuda", dtype=torch.uint8)
    y0, y1, x0, x1 = H // 12, H - H // 12, W // 6, W - W // 6                                     # the moving region
    fx[:, y0:y1, x0:x1] = 150
    box = motion_box(fx, fy)
    b = box.cpu().tolist()
    cw, ch = b[1] - b[0], b[3] - b[2]
    result = {"tool": "video_prep_rate", "device": torch.cuda.get_device_name(0), "frames": N, "height": H, "width": W, "reps": a.reps,
              "box": b, "passes": []}
    print("%d frames of %d x %d, box %s (crop %d x %d); median (best - worst) of %d calls" % (N, H, W, b, ch, cw, a.reps))

    # motion pass: both stacks read once, one flag byte per column per tile row and per row per tile column written
    ws = torch.empty(int(lib.viai_motion_box_ws_bytes(H, W)), dtype=torch.uint8, device="cuda")
    out_box = torch.empty(5, dtype=torch.int32, device="cuda")
    nbytes = 2 * N * H * W + ws.numel()
    t = timed(lambda: _lib.check(lib.viai_motion_flags(fx.data_ptr(), fy.data_ptr(), H * W, N, H, W, ws.data_ptr(), _stream()), "motion"), a.reps)
    result["passes"].append(entry("motion", t, nbytes, *copy_rate(nbytes, a.reps)))
    # box pass: the flags read once, five ints written
    nbytes = ws.numel() + 20
    t = timed(lambda: _lib.check(lib.viai_motion_box_of_flags(ws.data_ptr(), H, W, 50, out_box.data_ptr(), _stream()), "box"), a.reps)
    result["passes"].append(entry("box", t, nbytes, *copy_rate(nbytes, a.reps)))
    assert torch.equal(out_box, box)
    # prepare pass: the crop of every frame read once, the output written once (NCHW fp32, as VideoFrontEnd asks for it)
    for form, R, kw in (("train", 256, dict(crop_x=13, crop_y=21, flip=True)), ("eval", 224, {})):
        for what, frames, C in (("image", image, 3), ("flow", (fx, fy), 2)):
            nbytes = N * ch * cw * C + N * C * 224 * 224 * 4
            t = timed(lambda: prepare(frames, box, R, 224, nchw=True, **kw), a.reps)
            result["passes"].append(entry("prepare %s %s" % (form, what), t, nbytes, *copy_rate(nbytes, a.reps),
                                          extra={"R": R, "size": 224, "channels": C, "crop": [ch, cw]}))
    print(json.dumps(result, sort_keys=True))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(result, f, sort_keys=True, indent=1)


if __name__ == "__main__":
    main()
