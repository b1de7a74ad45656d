"""A numpy restatement of `_process_utterance` (utils/librivox.py:44-117) behind the file decode, shared by the preprocessing tests.

It restates the stages the two new kernels cover -- rescaling, chunking, the silence trim, the padded and cut signal -- with the frame
arithmetic of `viai_amd.audio`.  The functions that turn floats into classes / companded floats are PARAMETERS (`quantize`, `compand`): the GPU
tests pass the device's own `mulaw_quantize`, so that a comparison is exact and says nothing about how log1p rounds; the defaults are the closed
forms in float64.  The mel is not restated here: the tests compare it with `MelFrontEnd` on a fresh copy of the same samples, bit for bit.
"""
import numpy as np

from viai_amd.audio import lws_num_frames, lws_pad_lr


def mulaw_np(x, mu=255):
    x = np.asarray(x, dtype=np.float64)
    return np.sign(x) * np.log1p(mu * np.abs(x)) / np.log1p(mu)


def mulaw_quantize_np(x, mu=255):
    return np.clip(np.trunc((mulaw_np(x, mu) + 1) / 2 * mu), 0, mu).astype(np.int64)


def start_and_end(classes, thr, silence=127):
    """utils/audio.py:56-67 as loops, without the asserts: (start, end, ok)"""
    q = np.asarray(classes).astype(np.int64)
    start = q.size
    for i in range(q.size):
        if abs(int(q[i]) - silence) > thr:
            start = i
            break
    end = -1
    for i in range(q.size - 1, 1, -1):
        if abs(int(q[i]) - silence) > thr:
            end = i
            break
    return start, end, start < q.size and end >= 0


def rescale_np(wav, rescaling_max=0.999):
    """librivox.py:48-49 on a float32 array: numpy keeps float32, one rounding per operation"""
    wav = np.asarray(wav, dtype=np.float32)
    return wav / np.abs(wav).max() * np.float32(rescaling_max)


def chunks_np(n, chunk):
    k = n // chunk
    return [(i * chunk, n if i == k - 1 else (i + 1) * chunk) for i in range(k)]


def process_utterance_np(wav, input_type="mulaw-quantize", mu=255, thr=2, rescaling=True, rescaling_max=0.999, chunk=4096, fft=1024, hop=256,
                         quantize=None, compand=None):
    """-> one dict per chunk: chunk, start, end, wav (trimmed, rescaled), signal, timesteps, frames"""
    quantize = quantize or (lambda x: mulaw_quantize_np(x, mu))
    compand = compand or (lambda x: mulaw_np(x, mu).astype(np.float32))
    wav = np.asarray(wav, dtype=np.float32)
    if rescaling:
        wav = rescale_np(wav, rescaling_max)
    out = []
    for c, (a, b) in enumerate(chunks_np(wav.size, chunk)):
        w = wav[a:b]
        if input_type == "mulaw-quantize":
            q = np.asarray(quantize(w))
            start, end, ok = start_and_end(q, thr)
            assert ok, "chunk %d is silent" % c
            w, sig, pad = w[start:end], q[start:end].astype(np.int32), mu // 2
        else:
            start, end = 0, w.size
            sig, pad = (np.asarray(compand(w)) if input_type == "mulaw" else w), 0
        l, r = lws_pad_lr(w.size, fft, hop)
        N = lws_num_frames(w.size, fft, hop)
        sig = np.pad(sig, (l, r), mode="constant", constant_values=pad)
        assert sig.size >= N * hop
        out.append(dict(chunk=c, start=start, end=end, wav=w, signal=sig[:N * hop], timesteps=N * hop, frames=N))
    return out
