"""Shared by test_wav_io_cpu.py and test_wav_io_gpu.py: the PCM rule of include/viai_hip.h ("WAV in, WAV out") stated in numpy, and the case table.

The numpy statement uses numpy's own float32 arithmetic (one rounding per operation, conversions to nearest even) and shares no code with
csrc/viai_pcm_rule.h.  The mono downmix is an explicit loop over the channels, in order, not np.mean.  Every comparison made with it is for
equal bits."""
import os
import re
import struct

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
FORMATS = ("u8", "s16", "s24", "s32", "f32", "f64")
BYTES = {"u8": 1, "s16": 2, "s24": 3, "s32": 4, "f32": 4, "f64": 8}
BITS = {"u8": 8, "s16": 16, "s24": 24, "s32": 32}
T = int(re.search(r"#define\s+VIAI_PCM_TILE\s+(\d+)", open(os.path.join(ROOT, "include", "viai_hip.h")).read()).group(1))
CHANNELS = (1, 2, 3, 8)
FRAMES = (1, 15, 16, 17, T - 1, T, T + 1, 2 * T + 17)


# ----------------------------------------------------------------------------- the rule
def decode_rule(data, fmt, channels, mono=False):
    """1-D uint8 -> (channels | 1, frames) float32"""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    with np.errstate(all="ignore"):
        if fmt == "u8":
            x = (data.astype(np.int32) - 128).astype(f32) / f32(128)
        elif fmt == "s16":
            x = data.view("<i2").astype(f32) / f32(32768)
        elif fmt == "s24":
            b = data.reshape(-1, 3).astype(np.int32)
            v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
            v = (v ^ 0x800000) - 0x800000
            x = v.astype(f32) / f32(8388608)
        elif fmt == "s32":
            x = data.view("<i4").astype(f32) * f32(2.0 ** -31)
        elif fmt == "f32":
            x = data.view("<f4").copy()
        else:
            x = data.view("<f8").astype(f32)
        x = np.ascontiguousarray(x.reshape(-1, channels).T)
        if mono:
            acc = x[0].copy()
            for c in range(1, channels):
                acc = acc + x[c]
            x = (acc / f32(channels)).reshape(1, -1)
    return x


def encode_rule(wav, fmt):
    """(C, n) float32 -> 1-D uint8, the plain rule"""
    x = np.ascontiguousarray(np.asarray(wav, dtype=f32).T).reshape(-1)
    if fmt == "f32":
        return x.astype("<f4").view(np.uint8).copy()
    if fmt == "f64":
        return x.astype("<f8").view(np.uint8).copy()
    bits = BITS[fmt]
    scale = f32(2.0 ** (bits - 1))
    fin = np.isfinite(x)
    with np.errstate(all="ignore"):
        y = np.rint(np.where(fin, x, f32(0)) * scale)                     # float32 product, then ties to even
    q = np.clip(y.astype(np.float64), -(2.0 ** (bits - 1)), 2.0 ** (bits - 1) - 1).astype(np.int64)      # the clamp, in exact arithmetic
    q[~fin] = 0
    if fmt == "u8":
        return (q + 128).astype(np.uint8)
    if fmt == "s16":
        return q.astype("<i2").view(np.uint8).copy()
    if fmt == "s32":
        return q.astype("<i4").view(np.uint8).copy()
    u = (q & 0xFFFFFF).astype(np.uint32)
    return np.stack([u & 0xFF, (u >> 8) & 0xFF, (u >> 16) & 0xFF], 1).astype(np.uint8).reshape(-1)


def encode_norm_rule(wav):
    """(C, n) float32 -> 1-D uint8 of int16: the reference's save_wav, non-finite samples 0 and outside the peak"""
    x = np.ascontiguousarray(np.asarray(wav, dtype=f32).T).reshape(-1)
    fin = np.isfinite(x)
    peak = np.abs(x[fin]).max() if fin.any() else f32(0)
    scale = f32(3276700.0) if float(peak) <= 0.01 else f32(32767) / f32(peak)
    y = np.where(fin, x, f32(0)) * scale
    assert y.dtype == f32
    return np.trunc(y).astype(np.int64).astype("<i2").view(np.uint8).copy()


def patch_rule(data, wav, fmt, gaps):
    """a copy of data in which only the samples of the gaps are the plain encoding of wav"""
    C, n = wav.shape
    bps = BYTES[fmt]
    enc = encode_rule(wav, fmt).reshape(n, C, bps)
    out = np.array(data, dtype=np.uint8).reshape(n, C, bps)
    count, start, length = gaps
    K = start.shape[1]
    for c in range(C):
        for k in range(min(int(count[c]), K)):
            s, e = max(int(start[c, k]), 0), min(int(start[c, k]) + int(length[c, k]), n)
            if e > s:
                out[s:e, c] = enc[s:e, c]
    return out.reshape(-1)


# ----------------------------------------------------------------------------- the cases
def random_bytes(fmt, channels, frames):
    """seeded random sample bytes; the float formats without non-finite bit patterns"""
    rng = np.random.RandomState(1000 * FORMATS.index(fmt) + 100 * channels + frames % 97 + frames)
    data = rng.randint(0, 256, frames * channels * BYTES[fmt]).astype(np.uint8)
    if fmt == "f32":
        v = data.view("<u4")
        v[(v & 0x7F800000) == 0x7F800000] &= np.uint32(0xBFFFFFFF)
    if fmt == "f64":
        v = data.view("<u8")
        v[(v & np.uint64(0x7FF0000000000000)) == np.uint64(0x7FF0000000000000)] &= np.uint64(0xBFFFFFFFFFFFFFFF)
    return data


SPECIALS = np.array([1.0, -1.0, np.nextafter(f32(1), f32(2)), np.inf, -np.inf, np.nan, 0.5 / 32768, 1.5 / 32768, -0.5 / 32768, 2.5 / 128,
                     -1.5 / 8388608, 0.0, -0.0, 1e-40, 0.999999, -0.99999994, 3.0e38, -3.0e38, 127.5 / 128, 32766.5 / 32768], dtype=f32)


def random_wave(channels, frames, seed=0):
    """(channels, frames) float32 in about [-1.2, 1.2] with the special values sprinkled in"""
    rng = np.random.RandomState(7919 * channels + frames + 31 * seed)
    x = rng.uniform(-1.2, 1.2, (channels, frames)).astype(f32)
    flat = x.reshape(-1)
    at = rng.permutation(flat.size)[:min(flat.size // 2, SPECIALS.size)]
    flat[at] = SPECIALS[:at.size]
    return x


def gaps_case(channels, frames, variant=0, K=4):
    """count (C,), start (C, K), length (C, K) int32.  One kind of channel holds runs that touch sample 0, have length 0 and touch each other;
    the other kind runs that begin before the clip, reach past its end, and a count above K (the fifth run is not in the lists and is not
    patched).  `variant` swaps the kinds."""
    n = frames
    count = np.zeros(channels, dtype=np.int32)
    start = np.zeros((channels, K), dtype=np.int32)
    length = np.zeros((channels, K), dtype=np.int32)
    for c in range(channels):
        if (c + variant) % 2 == 0:
            runs, cnt = [(0, 3), (n // 3, 0), (n // 2, 2), (n // 2 + 2, 3)], 4
        else:
            runs, cnt = [(-3, 5), (n - 2, 5), (n // 2, 1), (n // 4, 2)], 5
        count[c] = cnt
        start[c], length[c] = [r[0] for r in runs], [r[1] for r in runs]
    return count, start, length


# ----------------------------------------------------------------------------- long clips
# pcm_encode_kernel's grid stops at 2048 blocks, so from 2048 T frames on a block walks a second tile: 2050 tiles put blocks 0 and 1 there, block 1
# on the 5-frame tail.  With normalize every block reads the per-tile peaks 256 at a time: above 256 tiles a thread reads more than one.
# pcm_patch_kernel lays 32 blocks of 256 along a run: a run longer than 8192 samples is walked in strides.
ENCODE_BLOCKS, PEAK_THREADS, PATCH_STRIDE = 2048, 256, 32 * 256
LONG_FRAMES = ENCODE_BLOCKS * T + T + 5
LONG_ENCODE = (("s16", 2), ("s24", 1), ("u8", 3), ("f32", 2))             # even frame bytes (the swizzled stage), odd, odd, a float format
PEAK_FRAMES = 299 * T + 5                                                 # 300 tiles: the peaks of tiles 256 .. 299 are a thread's second read
PEAK_TILES = ((PEAK_FRAMES, 0), (PEAK_FRAMES, 255), (PEAK_FRAMES, 256), (LONG_FRAMES, 2047), (LONG_FRAMES, 2049))
LONG_PATCH = (("s16", 2), ("s24", 1))
LONG_RUN = (2000003, 3 * PATCH_STRIDE + 77)


def peak_clip(frames, tile):
    """(1, frames) float32 within +-0.3 with the one peak, -0.9, in `tile` (its second frame) and a larger inf and a nan in two other tiles"""
    rng = np.random.RandomState(frames % 1000 + tile)
    x = rng.uniform(-0.3, 0.3, (1, frames)).astype(f32)
    ntiles = -(-frames // T)
    x[0, ((tile + 7) % ntiles) * T] = np.inf
    x[0, ((tile + 130) % ntiles) * T + 3] = np.nan
    x[0, tile * T + 1] = -0.9
    return x


def long_patch_gaps(channels, K=4):
    """the long run in the last channel, a short one in channel 0 (mono: both in channel 0), and entries behind count that must not be read"""
    count = np.zeros(channels, dtype=np.int32)
    start = np.full((channels, K), 5, dtype=np.int32)
    length = np.full((channels, K), 9, dtype=np.int32)
    short = (70001, 33)
    runs = [[short, LONG_RUN]] if channels == 1 else [[short]] + [[] for _ in range(channels - 2)] + [[LONG_RUN]]
    for c, r in enumerate(runs):
        count[c] = len(r)
        for k, (s, l) in enumerate(r):
            start[c, k], length[c, k] = s, l
    return count, start, length


def wav_file(fmt, channels, rate, data, extra_before=b"", extra_after=b"", tag=None, extensible=False, data_size=None):
    """the bytes of a RIFF/WAVE file around `data`, written out by hand"""
    bps = BYTES[fmt]
    tag = tag if tag is not None else (3 if fmt in ("f32", "f64") else 1)
    head = struct.pack("<HHIIHH", 0xFFFE if extensible else tag, channels, rate, rate * channels * bps, channels * bps, 8 * bps)
    if extensible:
        head += struct.pack("<HHI", 22, 8 * bps, 0) + struct.pack("<H", tag) + b"\x00\x00\x00\x00\x10\x00\x80\x00\x00\xaa\x00\x38\x9b\x71"
    data = bytes(data)
    size = len(data) if data_size is None else data_size
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(head)) + head + extra_before + b"data" + struct.pack("<I", size) + data + extra_after
    return b"RIFF" + struct.pack("<I", len(body)) + body


def chunk(cid, payload):
    """one RIFF chunk, the pad byte behind an odd size included"""
    return cid + struct.pack("<I", len(payload)) + payload + b"\0" * (len(payload) & 1)
