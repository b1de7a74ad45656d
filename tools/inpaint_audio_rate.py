"""Wall time of ONE `AudioInpainter` call at the native shape: 8 clips of n = 52 480 samples (80 mel bands x 208 frames at fft 1024 / hop 256), a
13 312-sample gap per clip at a start that is no multiple of the hop, the audio-only generator and the reference-size vocoder (24 layers / 512
residual / 512 gate / 256 skip channels, mixture of logistics).  Untrained weights: the time does not depend on them.  The call is the aligned
waveform, the frame mask, the mel front end, the generator, the composite and receptive field + gap = 505 + 13 312 vocoder steps of the chain form.

The measurement runs once, in a child process under a time limit, and the tool prints one JSON line; it makes no promise about the number.

    python tools/inpaint_audio_rate.py [--timeout 300]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, HOP, FRAMES_OF_SAMPLES, GAP = 8, 256, 205, 13312


def measure():
    sys.path.insert(0, ROOT)
    import torch
    from viai_amd import AudioInpainter
    from viai_amd.model import AudioModel, StepConfig
    from viai_amd.wavenet import WaveNet
    torch.manual_seed(1234)
    n = FRAMES_OF_SAMPLES * HOP
    hp = StepConfig()
    hp.cin_channels, hp.max_mel_lengths = 80, 208
    inp = AudioInpainter(AudioModel(hp, device="cuda:0"), WaveNet(dropout=0.0).cuda().eval())
    R = inp.vocoder.receptive_field
    wav = (torch.rand(B, n, device="cuda") * 2 - 1) * 0.5
    starts = [10000 + 1111 * b for b in range(B)]
    u = (torch.empty(B, R + GAP, 10, device="cuda").uniform_(1e-5, 1 - 1e-5), torch.empty(B, R + GAP, device="cuda").uniform_(1e-5, 1 - 1e-5))
    inp(wav[:, :8 * HOP].contiguous(), 700, 300)                         # warm-up: library load, first launches of every stage
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out, parts = inp(wav, starts, GAP, uniforms=u, return_parts=True)
    torch.cuda.synchronize()
    t = time.perf_counter() - t0
    print(json.dumps({"tool": "inpaint_audio_rate", "streams": B, "samples": n, "frames": int(parts["c"].size(2)), "num_mels": int(parts["c"].size(1)),
                      "gap_samples": GAP, "masked_frames": parts["frames"][1], "vocoder_steps": R + GAP, "call_s": round(t, 4),
                      "finite": bool(torch.isfinite(out).all())}, sort_keys=True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--timeout", type=float, default=300.0, help="seconds the one run may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return measure()
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], stdout=subprocess.PIPE, text=True, timeout=args.timeout)
    except subprocess.TimeoutExpired:
        print(json.dumps({"tool": "inpaint_audio_rate", "error": "no result within %g s" % args.timeout}))
        return 124
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    if r.returncode != 0 or not lines:
        print(json.dumps({"tool": "inpaint_audio_rate", "error": "the run ended with status %d" % r.returncode}))
        return r.returncode or 1
    print(lines[-1])
    return 0


if __name__ == "__main__":
    sys.exit(main())
