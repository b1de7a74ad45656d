#!/usr/bin/env python
"""Rate of the vocoder data preparation (viai_amd.preprocess) on a ten-minute synthetic file: seconds of audio prepared per second, the split
between the two new launches (viai_utt_trim_bounds, viai_utt_pack) and the mel launches they feed, and the same steps without the mel in numpy
on the CPU, and the mel stage both ways: one launch and one transpose per row (a front end without `ragged`) against the one ragged call
the preprocessor makes, each as best and worst of the repetitions.  No threshold: the figures go into DESIGN.md 11.2h / 11.2i.

    python tools/preprocess_rate.py [--minutes 10] [--reps 5]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def synthetic(n, sr, seed=0):
    """bursts of noise under a slow envelope with half a second of silence every four seconds: chunks start and end in silence"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sr
    env = np.clip(np.sin(2 * np.pi * t / 4.0) * 1.5, 0, 1) ** 2
    return (rng.standard_normal(n) * 0.2 * env).astype(np.float32)


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


def timed(fn, reps):
    return min(timed_all(fn, reps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=10.0)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    from preprocess_common import process_utterance_np
    from viai_amd import _lib
    from viai_amd.audio import AudioConfig, MelFrontEnd
    from viai_amd.preprocess import UtterancePreprocessor, chunk_bounds, trim_bounds
    sr = AudioConfig.sample_rate
    n = int(a.minutes * 60 * sr)
    host = synthetic(n, sr)
    wav = torch.from_numpy(host).cuda()
    front = MelFrontEnd(AudioConfig, device="cuda")
    pre = UtterancePreprocessor(front=front)
    recs = pre(wav)
    audio_s = n / sr
    whole = timed(lambda: pre(wav), a.reps)
    # the pieces, on the same buffers
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    chunks = chunk_bounds(n, pre.chunk_samples)
    amax = torch.zeros(1, device="cuda")
    lib.viai_absmax(wav.data_ptr(), n, amax.data_ptr(), st)
    t_amax = timed(lambda: lib.viai_absmax(wav.data_ptr(), n, amax.data_ptr(), st), a.reps)
    t_trim = timed(lambda: trim_bounds(wav, chunks, pre.silence_threshold, pre.mu, amax, pre.rescaling_max), a.reps)
    rows = [r.wav for r in recs]
    t_mel = timed(lambda: [front(r[None]) for r in rows], a.reps)
    # the mel stage as the preprocessor runs it: per row with its transpose (the loop a front end without `ragged` gets), and the one ragged call
    store = rows[0].untyped_storage()
    packed = torch.empty(0, dtype=torch.float32, device="cuda").set_(store, 0, (store.nbytes() // 4,))
    offs = [(r.data_ptr() - packed.data_ptr()) // 4 for r in rows]
    lens = [r.numel() for r in rows]
    t_loop = timed_all(lambda: [front(r[None])[0, 0].t().contiguous() for r in rows], a.reps)
    t_rag = timed_all(lambda: front.ragged(packed, lens, offs, time_major=True), a.reps)

    class Plain:
        cfg = front.cfg

        def __call__(self, w, mask=None):
            return front(w, mask)
    pre_loop = UtterancePreprocessor(front=Plain())
    t_whole = timed_all(lambda: pre(wav), a.reps)
    t_whole_loop = timed_all(lambda: pre_loop(wav), a.reps)
    t_pack = whole - t_amax - t_trim - min(t_rag)                 # the pack launch, its table upload and the bounds read
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def device_time(fn):
        fn(); torch.cuda.synchronize()
        ev0.record(); fn(); ev1.record(); torch.cuda.synchronize()
        return ev0.elapsed_time(ev1) * 1e-3
    d_trim = device_time(lambda: trim_bounds(wav, chunks, pre.silence_threshold, pre.mu, amax, pre.rescaling_max))
    d_mel = device_time(lambda: [front(r[None]) for r in rows])
    d_rag = device_time(lambda: front.ragged(packed, lens, offs, time_major=True))
    d_whole = device_time(lambda: pre(wav))
    t0 = time.perf_counter()
    ref = process_utterance_np(host, chunk=pre.chunk_samples)
    t_np = time.perf_counter() - t0
    same = all(r.start == w["start"] and r.end == w["end"] for r, w in zip(recs, ref))
    print("file: %.1f s of audio, %d chunks, %d pairs" % (audio_s, len(chunks), len(recs)))
    print("device, whole call (wall, best of %d): %.2f ms = %.0f s of audio per second" % (a.reps, whole * 1e3, audio_s / whole))
    print("  viai_absmax %.3f ms | viai_utt_trim_bounds %.3f ms | ragged mel call %.3f ms | pack + read + upload %.3f ms (by difference) | "
          "for comparison, %d one-row mel launches without their transposes: %.3f ms"
          % (t_amax * 1e3, t_trim * 1e3, min(t_rag) * 1e3, t_pack * 1e3, len(rows), t_mel * 1e3))
    ms = lambda v: "%.3f ms (worst of %d: %.3f)" % (min(v) * 1e3, len(v), max(v) * 1e3)
    print("  mel stage, %d rows: per-row launches + transposes %s | one ragged call %s" % (len(rows), ms(t_loop), ms(t_rag)))
    print("  whole call: per-row mel loop %s | ragged mel %s" % (ms(t_whole_loop), ms(t_whole)))
    print("  stream time (events): whole %.3f ms, trim_bounds %.3f ms, ragged mel call %.3f ms, the rest (absmax, pack) %.3f ms; %d one-row mel launches %.3f ms"
          % (d_whole * 1e3, d_trim * 1e3, d_rag * 1e3, (d_whole - d_trim - d_rag) * 1e3, len(rows), d_mel * 1e3))
    print("numpy on the CPU, same steps without the mel (fp64 mu-law): %.1f ms = %.0f s of audio per second; bounds %s the device's"
          % (t_np * 1e3, audio_s / t_np, "equal" if same else "DIFFER from"))


if __name__ == "__main__":
    main()
