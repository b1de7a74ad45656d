#!/usr/bin/env python
"""Generate tests/golden/preprocess.npz from the REFERENCE's own data-preparation functions (build container only).

Runs `utils.audio.start_and_end_indices`, `lws_num_frames` and `lws_pad_lr` (utils/audio.py:56-108) over a table of class sequences and lengths
chosen to hit every branch, and the chunk loop of `utils.librivox._process_utterance` (:44-117) in its "raw" form over four file lengths.  The
modules are imported by the stand-in-module recipe of tools/make_goldens.py (`loader_goldens`): none of the functions run here calls into lws,
librosa or nnmnkwii, so empty stand-ins make the imports succeed.  For the chunk loop the stand-ins are a HARNESS: `audio.load_wav` hands over a
ramp of the requested length, `audio.melspectrogram` records the length it was given and returns zeros of the right shape, `np.save` records.

The fixture is data only: the inputs and what the reference returned.  A row where the reference's asserts fire is recorded with ok = 0.

Run:  python tools/make_preprocess_golden.py            (needs /root/reference)
"""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(ROOT, "tools", "oracle_stubs"))
sys.path.insert(0, REF)
for name in ("lws", "librosa", "librosa.filters", "nnmnkwii", "nnmnkwii.preprocessing", "hparams", "audio", "wavenet_vocoder", "wavenet_vocoder.util"):
    sys.modules.setdefault(name, types.ModuleType(name))
sys.modules["nnmnkwii"].preprocessing = sys.modules["nnmnkwii.preprocessing"]

from utils import audio as RA          # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "preprocess.npz")
S = 127


def trim_cases():
    """name, thr, classes.  Silence is 127; `a` is a class clearly outside the band."""
    a = 200
    quiet = lambda n: [S] * n
    cases = []
    for thr in (0, 2, 5):
        edge_in, edge_out = S + thr, S + thr + 1                       # a deviation of exactly thr is silent, thr + 1 is not
        cases += [
            ("start0", thr, [a] + quiet(4) + [a] + quiet(3)),
            ("only01", thr, [a, a] + quiet(6)),
            ("only0", thr, [a] + quiet(7)),
            ("only1", thr, quiet(1) + [a] + quiet(6)),
            ("last_at_2", thr, [a, S, a] + quiet(5)),
            ("first_and_last_at_2", thr, [S, S, a] + quiet(5)),
            ("last_at_size_minus_1", thr, quiet(3) + [a] + quiet(3) + [a]),
            ("start0_last_size_minus_1", thr, [a] + quiet(6) + [a]),
            ("all_silent", thr, quiet(9)),
            ("all_active", thr, [a] * 9),
            ("single_active", thr, quiet(4) + [a] + quiet(4)),
            ("middle", thr, quiet(3) + [a, S, 30, a] + quiet(4)),
            ("edge_exact_is_silent", thr, [edge_in, S - thr] * 2 + [edge_out] + [S - thr, edge_in] + [S - thr - 1] + [edge_in, S - thr]),
            ("edge_only_exact", thr, [edge_in, S - thr] * 4),
            ("edge_plus_one_at_ends", thr, [edge_out] + [edge_in] * 5 + [S - thr - 1]),
            ("length3", thr, [S, a, a]),
            ("length3_last", thr, [a, S, a]),
        ]
    return cases


def layout_lengths(fft, hop):
    ls = set()
    for k in (1, 2, 4, 5, 16, 17):
        ls |= {k * hop, k * hop + 1, k * hop + hop - 1, k * hop - 1}
    ls |= {1, 2, 3, fft - 1, fft, fft + 1, 4095, 4097, 12345, 128000, 131071}
    return sorted(ls)


def chunk_run(n, sample_rate, fft, hop):
    """the reference's chunk loop over a file of n samples -> the lengths of the chunks it cut and the timesteps it reported"""
    hp = types.SimpleNamespace(rescaling=False, rescaling_max=0.999, sample_rate=sample_rate, input_type="raw", quantize_channels=256,
                               silence_threshold=2, fft_size=fft)
    sys.modules["hparams"].hparams = hp
    util = sys.modules["wavenet_vocoder.util"]
    util.is_mulaw_quantize = lambda s: s == "mulaw-quantize"
    util.is_mulaw = lambda s: s == "mulaw"
    util.is_raw = lambda s: s == "raw"
    seen = []
    au = sys.modules["audio"]
    au.load_wav = lambda path: np.arange(n, dtype=np.float32) / max(n, 1)
    au.get_hop_size = lambda: hop
    au.lws_pad_lr = RA.lws_pad_lr
    au.start_and_end_indices = RA.start_and_end_indices

    def mel(wav):
        seen.append((len(wav), float(wav[0]) if len(wav) else -1.0))
        return np.zeros((80, RA.lws_num_frames(len(wav), fft, hop)))
    au.melspectrogram = mel
    sys.modules.pop("utils.librivox", None)
    from utils import librivox as RL
    real_save = np.save
    np.save = lambda *a, **k: None
    try:
        res = RL._process_utterance("", 1, "", "t")
    finally:
        np.save = real_save
    first = [int(round(v * max(n, 1))) for _, v in seen]               # the ramp's value is the sample's index in the file
    return [s for s, _ in seen], first, [r[2] for r in res]


def main():
    out = {}
    cases = trim_cases()
    width = max(len(c) for _, _, c in cases)
    cls = np.full((len(cases), width), -1, dtype=np.int16)
    meta = np.zeros((len(cases), 5), dtype=np.int32)                   # thr, size, ok, start, end
    for i, (_, thr, c) in enumerate(cases):
        q = np.asarray(c, dtype=np.int64)
        cls[i, :len(c)] = q
        try:
            s, e = RA.start_and_end_indices(q, thr)
            meta[i] = (thr, len(c), 1, s, e)
        except AssertionError:
            meta[i] = (thr, len(c), 0, -1, -1)
    out["trim.names"] = np.array([n for n, _, _ in cases])
    out["trim.classes"] = cls
    out["trim.meta"] = meta
    rows = []
    for fft, hop in ((1024, 256), (1024, 320)):
        for n in layout_lengths(fft, hop):
            l, r = RA.lws_pad_lr(np.zeros(n, dtype=np.float32), fft, hop)
            rows.append((fft, hop, n, l, r, RA.lws_num_frames(n, fft, hop)))
    out["layout"] = np.asarray(rows, dtype=np.int64)                   # fft, hop, length, l, r, N
    chunk = 800                                                        # int(8.0 * 100)
    crow, clen, cfirst, csteps = [], [], [], []
    for n in (chunk - 1, chunk, chunk + 1, 3 * chunk + chunk // 2, 0, 2 * chunk - 1, 2 * chunk):
        lens, first, steps = chunk_run(n, 100, 1024, 256)
        crow.append((n, chunk, len(lens)))
        clen += lens; cfirst += first; csteps += steps
    out["chunks.files"] = np.asarray(crow, dtype=np.int64)             # n, chunk_samples, number of chunks
    out["chunks.length"] = np.asarray(clen, dtype=np.int64)            # per chunk, files concatenated
    out["chunks.first"] = np.asarray(cfirst, dtype=np.int64)
    out["chunks.timesteps"] = np.asarray(csteps, dtype=np.int64)
    np.savez_compressed(OUT, **out)
    print("preprocess -> %s (%.1f KB): %d trim rows (%d refused by the reference), %d layout rows, %d files / %d chunks"
          % (os.path.relpath(OUT, ROOT), os.path.getsize(OUT) / 1024, len(cases), int((meta[:, 2] == 0).sum()), len(rows), len(crow), len(clen)))


if __name__ == "__main__":
    main()
