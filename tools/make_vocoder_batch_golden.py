#!/usr/bin/env python
"""Generate tests/golden/vocoder_batch.npz from the REFERENCE's own `collate_fn` (Data_loaders/data_loader_utils.py:209-319; build container only).

The module is imported by the stand-in-module recipe of tools/make_preprocess_golden.py: `collate_fn` calls into none of lws, librosa, nnmnkwii,
sklearn or keras except `np_utils.to_categorical`, so empty stand-ins make the imports succeed and the one function is a HARNESS,
to_categorical(y, num_classes) = np.eye(num_classes)[y].  `np.int`, which :289 uses and numpy has removed, is put back as `int`.  The settings
of a case are written onto the module's `hparams` (and `hop_size` onto utils.audio's own copy, which `get_hop_size` reads); numpy's
`random.randint` is wrapped so that the crop draws of the reference are recorded.

The fixture is data only: inputs, seeds, settings, and what the reference returned (y, c, input_lengths, g) with the draws it made.  The dense input x
is not stored: the tool asserts that it is the one-hot of y with zero columns at t >= length (the float row itself for "raw"), the test rebuilds it.

Run:  python tools/make_vocoder_batch_golden.py [REFERENCE_DIR]       (default: $VIAI_REFERENCE, else ../reference next to the repository)
"""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("VIAI_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(ROOT, "tools", "oracle_stubs"))
sys.path.insert(0, REF)
for name in ("lws", "librosa", "librosa.filters", "nnmnkwii", "nnmnkwii.datasets", "sklearn", "sklearn.model_selection", "keras", "keras.utils",
             "keras.utils.np_utils"):
    sys.modules.setdefault(name, types.ModuleType(name))
sys.modules["nnmnkwii.datasets"].FileSourceDataset = sys.modules["nnmnkwii.datasets"].FileDataSource = object
sys.modules["sklearn.model_selection"].train_test_split = None
sys.modules["keras.utils"].np_utils = sys.modules["keras.utils.np_utils"]
sys.modules["keras.utils.np_utils"].to_categorical = lambda y, num_classes: np.eye(num_classes)[y]
if not hasattr(np, "int"):
    np.int = int

from Data_loaders import data_loader_utils as DL          # noqa: E402
from utils import audio as RA                             # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "vocoder_batch.npz")

# name: frames per row, hop, D, max_time_steps, max_time_sec, input_type, speaker ids, and how many different non-zero starts the seed has to
# give: two_draws pins the order of the draws, one_draw only that a draw is used at all
CASES = [
    dict(name="no_crop", frames=[3, 7, 5], hop=4, D=80),
    dict(name="crop", frames=[12, 5, 9, 20, 6], hop=4, D=80, max_time_steps=24, two_draws=True),         # L = 6: rows 0, 2, 3 are cropped, row 4 is exact
    dict(name="exact_is_not_cropped", frames=[6, 8], hop=4, D=6, max_time_steps=24, one_draw=True),
    dict(name="one_window_short", frames=[7, 10, 7], hop=4, D=6, max_time_steps=24, one_draw=True),                    # n - L == 1: start 0 whatever the seed
    dict(name="steps_not_divisible", frames=[9, 4, 13], hop=4, D=6, max_time_steps=27, two_draws=True),  # max_steps = 24
    dict(name="max_time_sec", frames=[11, 6, 15], hop=4, D=6, max_time_sec=0.0016, max_time_steps=8, two_draws=True),   # int(25.6) = 25 -> 24; sec wins
    dict(name="raw", frames=[5, 10, 8], hop=4, D=6, max_time_steps=24, input_type="raw"),
    dict(name="speaker_ids", frames=[4, 9, 6], hop=4, D=6, max_time_steps=20, speakers=[3, 0, 7], one_draw=True),
    dict(name="hop256", frames=[3, 7, 6], hop=256, D=80, max_time_steps=4 * 256 + 100, two_draws=True),
]


def inputs(case, seed):
    gen = np.random.RandomState(1000 + seed)
    raw = case.get("input_type", "mulaw-quantize") == "raw"
    rows = []
    for i, n in enumerate(case["frames"]):
        T = n * case["hop"]
        sig = (gen.randint(-2 ** 15, 2 ** 15, T) / 2.0 ** 15).astype(np.float32) if raw else gen.randint(0, 256, T).astype(np.int64)
        mel = (gen.randint(-512, 512, (n, case["D"])) / 64.0).astype(np.float32)
        rows.append((sig, mel, case["speakers"][i] if "speakers" in case else 0))
    return rows


def run(case, seed):
    """the reference's collate_fn on the case -> (x, y, c, g, lengths) as numpy arrays and the draws it made, as (high bound, value) pairs"""
    hp = DL.hparams
    hp.input_type = case.get("input_type", "mulaw-quantize")
    hp.quantize_channels = 256
    hp.max_time_sec = case.get("max_time_sec")
    hp.max_time_steps = case.get("max_time_steps")
    hp.hop_size = RA.hparams.hop_size = case["hop"]
    hp.sample_rate = 16000
    hp.upsample_conditional_features = True
    hp.cin_channels = case["D"]
    hp.gin_channels = 16 if "speakers" in case else -1
    draws = []
    real = np.random.randint

    def recording(low, high=None, *a, **k):
        v = real(low, high, *a, **k)
        draws.append((int(high), int(v)))
        return v
    np.random.seed(seed)
    np.random.randint = recording
    try:
        x, y, c, g, lengths = DL.collate_fn(inputs(case, seed))
    finally:
        np.random.randint = real
    return x.numpy(), y.numpy(), c.numpy(), None if g is None else g.numpy(), lengths.numpy(), draws


def starts_of(case, draws):
    """per row: the draw of a cropped row, 0 for the others (the reference draws for the rows with len(x) > max_steps, in batch order)"""
    mts = int(case["max_time_sec"] * 16000) if case.get("max_time_sec") is not None else case.get("max_time_steps")
    if mts is None:
        assert not draws
        return [0] * len(case["frames"])
    L = (mts - mts % case["hop"]) // case["hop"]
    it = iter(draws)
    out = []
    for n in case["frames"]:
        if n * case["hop"] > L * case["hop"]:
            high, v = next(it)
            assert high == n - L and 0 <= v < high
            out.append(v)
        else:
            out.append(0)
    assert next(it, None) is None
    return out


def main():
    out = {"names": np.array([c["name"] for c in CASES])}
    for case in CASES:
        name = case["name"]
        need = 2 if case.get("two_draws") else 1 if case.get("one_draw") else 0
        for seed in range(200):                                             # the first seed whose draws pin the order
            x, y, c, g, lengths, draws = run(case, seed)
            st = starts_of(case, draws)
            nz = sorted({s for s in st if s > 0})
            if len(nz) >= need:
                break
        else:
            raise AssertionError("%s: no seed below 200 gives %d different non-zero starts" % (name, need))
        assert len(nz) >= need, (name, st)
        rows = inputs(case, seed)
        B, T = y.shape[0], y.shape[1]
        assert y.shape == (B, T, 1) and c.shape[:2] == (B, case["D"]) and c.shape[2] * case["hop"] == T and T == lengths.max()
        if case.get("input_type", "mulaw-quantize") == "raw":
            assert x.shape == (B, 1, T) and y.dtype == np.float32 and np.array_equal(x[:, 0, :], y[:, :, 0])
        else:
            want = np.eye(256, dtype=np.float32)[y[:, :, 0]] * (np.arange(T)[None, :, None] < lengths[:, None, None])      # (B, T, K)
            assert x.shape == (B, 256, T) and y.dtype == np.int64 and np.array_equal(x, want.transpose(0, 2, 1))
        out[name + ".settings"] = np.asarray([case["hop"], case["D"], -1 if case.get("max_time_steps") is None else case["max_time_steps"], 16000, 256,
                                              seed], dtype=np.int64)                       # hop, D, max_time_steps (-1: None), sample_rate, K, seed
        out[name + ".max_time_sec"] = np.asarray(np.nan if case.get("max_time_sec") is None else case["max_time_sec"], dtype=np.float64)
        out[name + ".input_type"] = np.array(case.get("input_type", "mulaw-quantize"))
        out[name + ".n_frames"] = np.asarray(case["frames"], dtype=np.int64)
        sig = np.concatenate([r[0] for r in rows])
        out[name + ".signal"] = sig if sig.dtype == np.float32 else sig.astype(np.uint8)                # rows concatenated; classes fit a byte
        out[name + ".mel"] = np.concatenate([r[1] for r in rows])                                       # (sum of frames, D)
        if "speakers" in case:
            out[name + ".speakers"] = np.asarray(case["speakers"], dtype=np.int64)
            assert g is not None and g.tolist() == case["speakers"]
            out[name + ".g"] = g
        else:
            assert g is None
        out[name + ".draws"] = np.asarray(draws, dtype=np.int64).reshape(-1, 2)                         # (high bound, value), in the order drawn
        out[name + ".starts"] = np.asarray(st, dtype=np.int64)
        out[name + ".y"] = y if y.dtype == np.float32 else y.astype(np.uint8)
        out[name + ".c"] = c
        out[name + ".input_lengths"] = lengths
        print("%-22s seed %3d  starts %s  lengths %s" % (name, seed, st, lengths.tolist()))
    np.savez_compressed(OUT, **out)
    print("vocoder_batch -> %s (%.1f KB), %d cases" % (os.path.relpath(OUT, ROOT), os.path.getsize(OUT) / 1024, len(CASES)))


if __name__ == "__main__":
    main()
