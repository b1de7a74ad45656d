"""WAV in, WAV out: the bytes of an audio file <-> the (C, n) fp32 tensor the rest of the package takes (csrc/wav_io.hip).

    parse_wav        the RIFF header of a file or of its bytes -> WavInfo (pure Python)
    decode_pcm       interleaved little-endian sample bytes on the GPU -> planar fp32 (HIP); decode_pcm_host: the same rule in C++ on the host
    encode_pcm       planar fp32 -> sample bytes, plain or with the reference's peak normalisation (HIP); encode_pcm_host
    patch_pcm        re-encode ONLY the samples of detected gaps into a copy of the file's bytes (HIP); patch_pcm_host
    read_wav         file -> (wav, WavInfo), the data chunk copied to the device once
    write_wav        (C, n) or (n,) fp32 -> file; save_wav: the reference's name and rule (utils/audio.py:19-21)
    repair_file      read, find_gaps, repair, patch, write: every byte of the file outside the detected gaps keeps its value

The rule (include/viai_hip.h states it in full; csrc/viai_pcm_rule.h is its one implementation): U8 (b - 128) / 128, S16 v / 2^15, S24 v / 2^23,
S32 (float)v 2^-31, F32 the bits, F64 the C cast; encoding rounds to nearest even and clamps, a non-finite sample encodes as 0.  Decoding and
then encoding returns the bytes for U8, S16, S24 and F32 but NOT for S32 (fp32 holds 24 of its 32 bits) or F64: a file is therefore never
re-encoded as a whole by `repair_file`, only patched.
"""
from __future__ import annotations

import ctypes as C
import struct
from collections import namedtuple

import torch

from . import _lib
from .gap_detect import Gaps, find_gaps, repair

TILE = 1024                                              # VIAI_PCM_TILE of include/viai_hip.h: the frames one block owns
FORMATS = ("u8", "s16", "s24", "s32", "f32", "f64")      # the enum VIAI_PCM_* in order
BYTES = {"u8": 1, "s16": 2, "s24": 3, "s32": 4, "f32": 4, "f64": 8}

WavInfo = namedtuple("WavInfo", ("sample_rate", "channels", "fmt", "frames", "data_offset", "data_bytes"))
WavInfo.__doc__ = """fmt is one of FORMATS; frames whole frames lie in the data_bytes bytes at data_offset of the file (a trailing partial frame
is not counted in either)."""


def _fmt(fmt, what):
    if fmt not in FORMATS:
        raise ValueError("%s: format %r; one of %s" % (what, fmt, ", ".join(FORMATS)))
    return FORMATS.index(fmt)


def _channels(channels, what):
    if int(channels) != channels or not 1 <= channels <= 8:
        raise ValueError("%s: %r channels; 1 to 8" % (what, channels))
    return int(channels)


# ------------------------------------------------------------------------------------------------ the header
def parse_wav(path_or_bytes):
    """The header of a RIFF/WAVE file, given as a path or as bytes -> WavInfo.  Walks the chunks: unknown ones are skipped (with the pad byte
    behind an odd size), the first `fmt ` and the first `data` count.  Format tag 1 with 8, 16, 24 or 32 bits, 3 with 32 or 64 bits, 0xFFFE
    (extensible) resolved by the first two bytes of its sub-format.  A data size of 0 or 0xFFFFFFFF (a streamed file whose writer never came
    back) or one that runs past the end of the file means "to the end of the file"; a trailing partial frame is dropped.  ValueError names
    anything else: RF64, big-endian RIFX, a compressed tag, block_align != channels * bytes, more than 8 channels."""
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
        buf = bytes(path_or_bytes)
    else:
        with open(path_or_bytes, "rb") as f:
            buf = f.read()
    if len(buf) < 12:
        raise ValueError("parse_wav: %d bytes are no RIFF header" % len(buf))
    magic, form = buf[:4], buf[8:12]
    if magic in (b"RF64", b"BW64"):
        raise ValueError("parse_wav: %s (64-bit sizes) is not supported" % magic.decode())
    if magic == b"RIFX":
        raise ValueError("parse_wav: RIFX (big-endian) is not supported")
    if magic != b"RIFF" or form != b"WAVE":
        raise ValueError("parse_wav: not a RIFF/WAVE file (%r, %r)" % (magic, form))
    pos, fmt = 12, None
    while pos + 8 <= len(buf):
        cid, size = buf[pos:pos + 4], struct.unpack_from("<I", buf, pos + 4)[0]
        body = pos + 8
        if cid == b"fmt " and fmt is None:
            if size < 16 or body + 16 > len(buf):
                raise ValueError("parse_wav: a fmt chunk of %d bytes" % size)
            tag, channels, rate, _, align, bits = struct.unpack_from("<HHIIHH", buf, body)
            if tag == 0xFFFE:
                if size < 40 or body + 40 > len(buf):
                    raise ValueError("parse_wav: an extensible fmt chunk of %d bytes" % size)
                tag = struct.unpack_from("<H", buf, body + 24)[0]
            name = {(1, 8): "u8", (1, 16): "s16", (1, 24): "s24", (1, 32): "s32", (3, 32): "f32", (3, 64): "f64"}.get((tag, bits))
            if name is None:
                raise ValueError("parse_wav: format tag 0x%04x with %d bits per sample; PCM (1) with 8, 16, 24 or 32 bits and IEEE float (3) "
                                 "with 32 or 64 bits are supported" % (tag, bits))
            if not 1 <= channels <= 8:
                raise ValueError("parse_wav: %d channels; 1 to 8" % channels)
            if align != channels * BYTES[name]:
                raise ValueError("parse_wav: block_align %d, %d channels of %d bytes" % (align, channels, BYTES[name]))
            if rate < 1:
                raise ValueError("parse_wav: sample rate %d" % rate)
            fmt = (rate, channels, name)
        elif cid == b"data":
            if fmt is None:
                raise ValueError("parse_wav: the data chunk comes before any fmt chunk")
            left = len(buf) - body
            if size == 0 or size == 0xFFFFFFFF or size > left:
                size = left
            fb = fmt[1] * BYTES[fmt[2]]
            frames = size // fb
            return WavInfo(fmt[0], fmt[1], fmt[2], frames, body, frames * fb)
        pos = body + size + (size & 1)
    raise ValueError("parse_wav: no data chunk" if fmt is not None else "parse_wav: no fmt chunk")


def wav_header(sample_rate, channels, fmt, frames):
    """the bytes in front of the samples as `write_wav` lays them out: a 16-byte fmt chunk (tag 1) for the integer formats, as
    scipy.io.wavfile.write does it and as the stdlib `wave` module reads it; tag 3 with an 18-byte fmt chunk and a fact chunk for the float
    formats, scipy's layout for them.  A data chunk of odd size is followed by one pad byte, which the RIFF size counts."""
    _fmt(fmt, "wav_header")
    channels = _channels(channels, "wav_header")
    bps = BYTES[fmt]
    nbytes = frames * channels * bps
    if frames < 0 or nbytes + (nbytes & 1) + 64 > 0xFFFFFFFF:
        raise ValueError("wav_header: %d frames of %d bytes do not fit a RIFF file" % (frames, channels * bps))
    is_float = fmt in ("f32", "f64")
    head = struct.pack("<HHIIHH", 3 if is_float else 1, channels, sample_rate, sample_rate * channels * bps, channels * bps, 8 * bps)
    if is_float:
        body = b"fmt " + struct.pack("<I", 18) + head + struct.pack("<H", 0) + b"fact" + struct.pack("<II", 4, frames)
    else:
        body = b"fmt " + struct.pack("<I", 16) + head
    body = b"WAVE" + body + b"data" + struct.pack("<I", nbytes)
    return b"RIFF" + struct.pack("<I", len(body) + nbytes + (nbytes & 1)) + body


# ------------------------------------------------------------------------------------------------ the device calls
def _device_only(t, what):
    if not t.is_cuda:
        raise _lib.ViaiLibraryError("%s runs on the GPU only; no CPU fallback (%s_host states the rule on the host)" % (what, what))


def _bytes_tensor(data, fb, what):
    if data.dim() != 1 or data.dtype != torch.uint8:
        raise ValueError("%s: the data is a 1-D uint8 tensor" % what)
    if data.numel() % fb:
        raise ValueError("%s: %d bytes are no whole number of %d-byte frames" % (what, data.numel(), fb))
    return data.numel() // fb


def _planes(wav, what):
    if wav.dim() == 1:
        wav = wav.reshape(1, -1)
    if wav.dim() != 2:
        raise ValueError("%s: wav is (C, n) or (n,)" % what)
    _channels(wav.size(0), what)
    return wav


def _rows(wav):
    """fp32 with contiguous rows -> (tensor, stride in floats)"""
    wav = wav.float()
    if wav.size(1) > 0 and (wav.stride(1) != 1 or (wav.size(0) > 1 and wav.stride(0) < wav.size(1))):
        wav = wav.contiguous()
    return wav, (wav.stride(0) if wav.size(0) > 1 else max(wav.size(1), 1))


def _aligned16(data):
    """the kernels take the byte stream 16-byte aligned (a data chunk in its own allocation is); a view at another offset is copied"""
    data = data.contiguous()
    return data if data.data_ptr() % 16 == 0 else data.clone()


def decode_pcm(data_u8, fmt, channels, mono=False):
    """data_u8: 1-D uint8 on the GPU, frames x channels interleaved little-endian samples -> (channels, frames) fp32, or (1, frames) with
    mono=True (the channels added in order in fp32, then one division by the count).  One launch; a view that does not start 16-byte aligned
    is copied first.  ViaiLibraryError for a CPU tensor."""
    f = _fmt(fmt, "decode_pcm")
    channels = _channels(channels, "decode_pcm")
    frames = _bytes_tensor(data_u8, channels * BYTES[fmt], "decode_pcm")
    _device_only(data_u8, "decode_pcm")
    out = torch.empty(1 if mono else channels, frames, dtype=torch.float32, device=data_u8.device)
    if frames:
        from .ops import _stream
        data = _aligned16(data_u8)
        _lib.check(_lib.load().viai_pcm_decode(data.data_ptr(), f, channels, frames, int(bool(mono)), out.data_ptr(), frames, _stream()),
                   "viai_pcm_decode")
    return out


def encode_pcm(wav, fmt="s16", normalize=False):
    """wav (C, n) or (n,) fp32 on the GPU -> 1-D uint8 of n x C interleaved samples.  normalize=True (s16 only) is the reference's save_wav:
    scale by 32767 / max(0.01, peak) and truncate; two launches, the peak never leaves the device."""
    f = _fmt(fmt, "encode_pcm")
    wav = _planes(wav, "encode_pcm")
    if normalize and fmt != "s16":
        raise ValueError("encode_pcm: normalize is the reference's int16 rule; fmt is %r" % fmt)
    _device_only(wav, "encode_pcm")
    channels, frames = wav.shape
    dst = torch.empty(frames * channels * BYTES[fmt], dtype=torch.uint8, device=wav.device)
    if frames:
        from .ops import _stream
        lib = _lib.load()
        wav, stride = _rows(wav)
        ws = torch.empty(lib.viai_pcm_ws_bytes(frames) // 4, dtype=torch.float32, device=wav.device) if normalize else None
        _lib.check(lib.viai_pcm_encode(wav.data_ptr(), stride, channels, frames, f, int(bool(normalize)), dst.data_ptr(),
                                       None if ws is None else ws.data_ptr(), _stream()), "viai_pcm_encode")
    return dst


def _gap_tensors(gaps, channels, what):
    count, start, length = (torch.as_tensor(x) for x in Gaps(*gaps))
    if count.dim() != 1 or count.numel() != channels or start.dim() != 2 or start.size(0) != channels or start.shape != length.shape or \
            start.size(1) < 1:
        raise ValueError("%s: gaps are (count (C,), start (C, K), length (C, K)) with C = %d" % (what, channels))
    return count, start, length


def patch_pcm(data_u8, wav, fmt, gaps):
    """A clone of data_u8 (the file's sample bytes, 1-D uint8 on the GPU) in which ONLY the samples of `gaps` are re-encoded, plain rule, from
    wav (C, n): gap k of channel c covers frames [start[c][k], start[c][k] + length[c][k]), clamped to the clip, for k < min(count[c], K).
    `gaps` is a `Gaps` as `find_gaps` leaves it and is read on the device: nothing comes to the host.  Every other byte is the input's."""
    f = _fmt(fmt, "patch_pcm")
    wav = _planes(wav, "patch_pcm")
    channels, frames = wav.shape
    if _bytes_tensor(data_u8, channels * BYTES[fmt], "patch_pcm") != frames:
        raise ValueError("patch_pcm: %d bytes, wav holds %d frames of %d channels" % (data_u8.numel(), frames, channels))
    count, start, length = _gap_tensors(gaps, channels, "patch_pcm")
    _device_only(data_u8, "patch_pcm")
    _device_only(wav, "patch_pcm")
    dev = data_u8.device
    out = data_u8.clone(memory_format=torch.contiguous_format)
    if frames:
        from .ops import _stream
        wav, stride = _rows(wav)
        count, start, length = (x.to(device=dev, dtype=torch.int32).contiguous() for x in (count, start, length))
        _lib.check(_lib.load().viai_pcm_patch(wav.data_ptr(), stride, channels, frames, f, count.data_ptr(), start.data_ptr(), length.data_ptr(),
                                              start.size(1), out.data_ptr(), _stream()), "viai_pcm_patch")
    return out


# ------------------------------------------------------------------------------------------------ the host mirrors
def _np_bytes(data, fb, what):
    import numpy as np
    data = np.ascontiguousarray(np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.asarray(data))
    if data.ndim != 1 or data.dtype != np.uint8:
        raise ValueError("%s: the data is a 1-D uint8 array" % what)
    if data.size % fb:
        raise ValueError("%s: %d bytes are no whole number of %d-byte frames" % (what, data.size, fb))
    return data, data.size // fb


def _np_planes(wav, what):
    import numpy as np
    wav = np.ascontiguousarray(wav, dtype=np.float32)
    if wav.ndim == 1:
        wav = wav.reshape(1, -1)
    if wav.ndim != 2:
        raise ValueError("%s: wav is (C, n) or (n,)" % what)
    _channels(wav.shape[0], what)
    return wav


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def decode_pcm_host(data_u8, fmt, channels, mono=False):
    """`decode_pcm` on the host: a 1-D uint8 numpy array (or bytes) -> (channels | 1, frames) fp32 numpy array, plain C++ from the same rule
    header (`viai_pcm_decode_host`).  Needs the built library, not a GPU."""
    import numpy as np
    f = _fmt(fmt, "decode_pcm_host")
    channels = _channels(channels, "decode_pcm_host")
    data, frames = _np_bytes(data_u8, channels * BYTES[fmt], "decode_pcm_host")
    out = np.empty((1 if mono else channels, frames), dtype=np.float32)
    if frames:
        _lib.check(_lib.load().viai_pcm_decode_host(_vp(data), f, channels, frames, int(bool(mono)), _vp(out), frames), "viai_pcm_decode_host")
    return out


def encode_pcm_host(wav, fmt="s16", normalize=False):
    """`encode_pcm` on the host: (C, n) or (n,) fp32 numpy array -> 1-D uint8 numpy array (`viai_pcm_encode_host`)."""
    import numpy as np
    f = _fmt(fmt, "encode_pcm_host")
    wav = _np_planes(wav, "encode_pcm_host")
    if normalize and fmt != "s16":
        raise ValueError("encode_pcm_host: normalize is the reference's int16 rule; fmt is %r" % fmt)
    channels, frames = wav.shape
    dst = np.empty(frames * channels * BYTES[fmt], dtype=np.uint8)
    if frames:
        _lib.check(_lib.load().viai_pcm_encode_host(_vp(wav), frames, channels, frames, f, int(bool(normalize)), _vp(dst)), "viai_pcm_encode_host")
    return dst


def patch_pcm_host(data_u8, wav, fmt, gaps):
    """`patch_pcm` on the host (`viai_pcm_patch_host`): numpy arrays in, a patched copy of data_u8 out."""
    import numpy as np
    f = _fmt(fmt, "patch_pcm_host")
    wav = _np_planes(wav, "patch_pcm_host")
    channels, frames = wav.shape
    data, have = _np_bytes(data_u8, channels * BYTES[fmt], "patch_pcm_host")
    if have != frames:
        raise ValueError("patch_pcm_host: %d bytes, wav holds %d frames of %d channels" % (data.size, frames, channels))
    count, start, length = (np.ascontiguousarray(torch.as_tensor(x).cpu().numpy(), dtype=np.int32) for x in Gaps(*gaps))
    if count.shape != (channels,) or start.ndim != 2 or start.shape[0] != channels or start.shape != length.shape or start.shape[1] < 1:
        raise ValueError("patch_pcm_host: gaps are (count (C,), start (C, K), length (C, K)) with C = %d" % channels)
    out = data.copy()
    if frames:
        _lib.check(_lib.load().viai_pcm_patch_host(_vp(wav), frames, channels, frames, f, _vp(count), _vp(start), _vp(length), start.shape[1],
                                                   _vp(out)), "viai_pcm_patch_host")
    return out


# ------------------------------------------------------------------------------------------------ files
def _data_tensor(buf, info, device):
    """the data chunk of the file bytes as a uint8 tensor on `device`: one host-to-device copy, into an allocation of its own"""
    import numpy as np
    return torch.from_numpy(np.frombuffer(buf, dtype=np.uint8, count=info.data_bytes, offset=info.data_offset).copy()).to(device)


def read_wav(path, device="cuda", mono=False):
    """path -> (wav (channels | 1, frames) fp32 on `device`, WavInfo).  The data chunk goes to the device once and is decoded there.  The
    reference's `load_wav` (librosa.load at the configured rate) is `read_wav(path, mono=True)` followed by `Resampler(info.sample_rate, rate)`
    when the rates differ: libsndfile's integer scalings, librosa.to_mono's mean over channels, and this package's own resampler."""
    with open(path, "rb") as f:
        buf = f.read()
    info = parse_wav(buf)
    return decode_pcm(_data_tensor(buf, info, device), info.fmt, info.channels, mono=mono), info


def write_wav(path, wav, sample_rate, fmt="s16", normalize=False):
    """wav (C, n) or (n,) fp32 on the GPU -> a RIFF/WAVE file (`wav_header` for the layout).  Encoded on the device, one copy to the host."""
    wav = _planes(wav, "write_wav")
    if int(sample_rate) != sample_rate or not 1 <= sample_rate <= 0xFFFFFFFF:
        raise ValueError("write_wav: sample_rate is a positive integer")
    data = encode_pcm(wav, fmt, normalize=normalize).cpu().numpy().tobytes()
    with open(path, "wb") as f:
        f.write(wav_header(int(sample_rate), wav.size(0), fmt, wav.size(1)) + data + b"\0" * (len(data) & 1))


def save_wav(wav, path, sample_rate=16000):
    """The reference's `save_wav(wav, path)` (utils/audio.py:19-21): int16 after scaling by 32767 / max(0.01, max |wav|), truncated.  UNLIKE the
    reference it does not scale the caller's tensor in place: wav is only read.  Every sample of the clip changes under this rule; a repaired
    file that should keep its samples goes through `repair_file`."""
    write_wav(path, wav, sample_rate, "s16", normalize=True)


def repair_file(inpainter, src, dst, max_gaps=16, ar_below=0, ar_order=32, ar_context=1024, ar_method="burg", ar_iters=None,
                **find_gaps_kwargs):
    """Repair the WAV file `src` into `dst`; returns (Gaps, WavInfo).  Channels are rows of one `repair` call.  ar_below / ar_order /
    ar_context / ar_method / ar_iters go to `repair` as they are (0, the default: every gap goes to the inpainter); the autoregressive fill sees the file's own
    length, so its contexts never reach into the zero padding of step 3.

        1  read_wav(src, mono=False); a channel count the inpainter cannot take as rows (not 1, 2, 4 or 8) raises before any work
        2  find_gaps on the clip at its own length
        3  zero-pad to a whole number of hops AFTER detection: the padding is never a gap
        4  repair(..., sample_rate=the file's)        5  crop to the file's length
        6  patch_pcm into the file's own sample bytes 7  dst = src's header and chunks around the patched data chunk

    Every byte of dst outside the samples of the detected gaps equals src, for all six formats: header, other chunks, the other channels'
    samples inside a gap's frames, and a trailing partial frame.  An overflowing detection (count > max_gaps) raises as `repair` does and
    nothing is written.  `inpainter` is only called (as `repair` and `inpaint_at_rate` call it) and asked for `front.cfg.sample_rate` and
    `front.cfg.hop_size`.  Recordings too long for one inpainter call are not windowed here: its errors pass through."""
    cfg = inpainter.front.cfg
    rate, hop = int(cfg.sample_rate), int(cfg.hop_size)
    with open(src, "rb") as f:
        buf = f.read()
    info = parse_wav(buf)
    n = info.frames
    if info.channels not in (1, 2, 4, 8):
        raise ValueError("repair_file: %d channels; the inpainter takes 1, 2, 4 or 8 rows" % info.channels)
    if n < 1:
        raise ValueError("repair_file: %s holds no samples" % src)
    data = _data_tensor(buf, info, "cuda")
    wav = decode_pcm(data, info.fmt, info.channels)
    gaps = find_gaps(wav, max_gaps=max_gaps, **find_gaps_kwargs)
    if info.sample_rate == rate and n % hop:
        padded = torch.nn.functional.pad(wav, (0, hop - n % hop))
    else:
        padded = wav                                                        # at another rate inpaint_at_rate pads on the front end's grid
    if ar_below:
        out, _ = repair(inpainter, padded, gaps=gaps, sample_rate=info.sample_rate, ar_below=ar_below, ar_order=ar_order,
                        ar_context=ar_context, ar_lengths=[n] * info.channels, ar_method=ar_method, ar_iters=ar_iters)
    else:
        out, _ = repair(inpainter, padded, gaps=gaps, sample_rate=info.sample_rate)
    patched = patch_pcm(data, out[:, :n], info.fmt, gaps).cpu().numpy().tobytes()
    end = info.data_offset + info.data_bytes
    with open(dst, "wb") as f:
        f.write(buf[:info.data_offset] + patched + buf[end:])
    return gaps, info
