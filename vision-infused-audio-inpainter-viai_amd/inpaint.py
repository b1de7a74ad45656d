"""Inpainting a waveform end to end: mel front end, generator and vocoder in one call.

`AudioModel.test()` fills the masked frames of a mel spectrogram and `wavenet.inpaint_waveform` regenerates the samples of a gap from a conditioning
mel of the whole clip.  `AudioInpainter` is the join: it produces that mel.  What the join has to get right (include/viai_hip.h):

    alignment   MelFrontEnd follows lws: frames = n / hop + 3, frame j reads samples [j hop - l, j hop + hop), l = fft - hop.  The vocoder needs
                n == frames * hop, so the clip moves right by l silent samples (utils/librivox.py:92-102); aligned coordinate a = i + l.  Frame j
                then owns [j hop, (j + 1) hop) and its analysis window is [j hop, j hop + fft).                              (viai_wav_align)
    widening    a frame is damaged when its WINDOW meets the gap [a0, a1): j hop < a1 and j hop + fft > a0.  That is the gap's own frames and
                fft / hop - 1 more on the left; a mask as wide as the sample gap would hand the generator frames computed from silenced samples
                as known.                                                                                   (gap_frames, viai_gap_frame_mask)
    composite   the vocoder is conditioned on the real mel where frames are clean and on the generator's only where they are damaged: a select,
                so clean frames keep their bits.                                                                          (viai_mel_compose)
    samples     gaps are given in samples; `inpaint_waveform(..., gap_unit="samples")` takes them as they are.
"""
from __future__ import annotations

import torch

from . import _lib
from .audio import AudioConfig, MelFrontEnd
from .ops import _stream
from .wavenet_inpaint import _per_stream, hop_size, inpaint_waveform

STREAM_COUNTS = (1, 2, 4, 8)                 # the chain forms of incremental_forward, which a masked call runs


def gap_frames(a0, a1, fft, hop, frames):
    """The frames a gap damages.  [a0, a1) in ALIGNED samples (the clip's own index + fft - hop); frame j's analysis window is
    [j * hop, j * hop + fft), and it is damaged when the two meet: j * hop < a1 and j * hop + fft > a0, i.e. (a0 - fft) // hop < j < ceil(a1 / hop).
    Returns (first, count), clipped to [0, frames); an empty gap (a1 <= a0) or one that meets no frame gives (0, 0).
    Two ints for int arguments; two lists, one entry per stream, for sequences or tensors.  Pure host arithmetic."""
    if fft < 1 or hop < 1 or frames < 0:
        raise ValueError("gap_frames: fft >= 1, hop >= 1, frames >= 0")
    lo = torch.as_tensor(a0).detach().cpu().to(torch.int64).reshape(-1)
    hi = torch.as_tensor(a1).detach().cpu().to(torch.int64).reshape(-1)
    if lo.numel() != hi.numel():
        raise ValueError("gap_frames: a0 and a1 hold one entry per stream")
    first = (torch.div(lo - fft, hop, rounding_mode="floor") + 1).clamp(min=0)
    end = (-torch.div(-hi, hop, rounding_mode="floor")).clamp(max=frames)
    hit = (hi > lo) & (end > first)
    first, count = (first * hit).tolist(), ((end - first) * hit).tolist()
    if isinstance(a0, int) and isinstance(a1, int):
        return first[0], count[0]
    return first, count


def generator_width_rule(frames, video_frames=None):
    """The widths the generator (networks.MelEncoder / MelDecoder) accepts, or the reason it does not.  The encoder's 3x3 convs (padding 1) halve the
    width four times, w -> (w - 1) // 2 + 1 (MelEncoder.STRIDES, the second one has stride 1 in time), and the decoder resizes to each encoder map
    again, so audio alone takes every width >= 1.  With the visual branch the video feature of N frames, halved twice the same way
    (ImageEmbedding2.conv_1 / conv_2), is concatenated to the bottleneck and must be exactly as wide.  Returns None or a message."""
    def halve(w, times):
        for _ in range(times):
            w = (w - 1) // 2 + 1
        return w
    if frames < 1:
        return "the generator needs at least one frame"
    if video_frames is not None and halve(int(video_frames), 2) != halve(frames, 4):
        return ("%d frames give a bottleneck %d steps wide (four stride-2 convs, w -> (w - 1) // 2 + 1) but %d video frames give %d (two of them): "
                "MelDecoderImage concatenates the two, so they must agree (N = frames / 4)"
                % (frames, halve(frames, 4), int(video_frames), halve(int(video_frames), 2)))
    return None


def _i32(x, dev):
    return x.to(torch.int32).to(dev).contiguous()


def wav_align(wav, a0, a1, lpad):
    """`viai_wav_align`: wav (B, n) fp32 on the GPU, a0 / a1 (B,) int32 on the GPU (aligned coordinates) -> (B, n + lpad): lpad zeros in front, zeros
    in [a0, a1), every other sample bit for bit."""
    if not wav.is_cuda:
        raise _lib.ViaiLibraryError("wav_align runs on the GPU only; no CPU fallback")
    wav = wav.float().contiguous()
    B, n = wav.shape
    out = torch.empty(B, n + int(lpad), device=wav.device)
    _lib.check(_lib.load().viai_wav_align(wav.data_ptr(), a0.data_ptr(), a1.data_ptr(), out.data_ptr(), B, n, int(lpad), _stream()), "viai_wav_align")
    return out


def gap_frame_mask(a0, a1, frames, fft, hop):
    """`viai_gap_frame_mask`: a0 / a1 (B,) int32 on the GPU -> the (B, 1, 1, frames) time mask, 0 on the frames whose window meets [a0, a1)."""
    if not a0.is_cuda:
        raise _lib.ViaiLibraryError("gap_frame_mask runs on the GPU only; no CPU fallback")
    B = a0.numel()
    mask = torch.empty(B, 1, 1, int(frames), device=a0.device)
    _lib.check(_lib.load().viai_gap_frame_mask(a0.data_ptr(), a1.data_ptr(), mask.data_ptr(), B, int(frames), int(fft), int(hop), _stream()),
               "viai_gap_frame_mask")
    return mask


def mel_compose(real, fake, mask):
    """`viai_mel_compose`: real, fake (B, 1, F, T), mask (B, 1, 1, T) -> c (B, F, T) = real where mask != 0, fake elsewhere (a select: bits survive)."""
    if not real.is_cuda:
        raise _lib.ViaiLibraryError("mel_compose runs on the GPU only; no CPU fallback")
    if real.dim() != 4 or real.size(1) != 1 or fake.shape != real.shape or mask.numel() != real.size(0) * real.size(3):
        raise ValueError("mel_compose: real, fake (B, 1, F, T) and mask (B, 1, 1, T)")
    real, fake, mask = real.float().contiguous(), fake.float().contiguous(), mask.float().contiguous()
    B, _, F, T = real.shape
    c = torch.empty(B, F, T, device=real.device)
    _lib.check(_lib.load().viai_mel_compose(real.data_ptr(), fake.data_ptr(), mask.data_ptr(), c.data_ptr(), B, F, T, _stream()), "viai_mel_compose")
    return c


class AudioInpainter:
    """model: an `AudioModel`; vocoder: a `wavenet.WaveNet`, scalar-input or one-hot; front: a `MelFrontEnd` (default: one built from `AudioConfig`
    on the model's device).  The three must agree on the frame grid: ValueError when the vocoder's hop (the product of its up-sampling strides) is
    not the front end's, or its conditioning channels are not the front end's mel bands."""

    def __init__(self, model, vocoder, front=None):
        if front is None:
            front = MelFrontEnd(AudioConfig, device=model.device)
        cfg = front.cfg
        if hop_size(vocoder) != cfg.hop_size:
            raise ValueError("AudioInpainter: the vocoder up-samples a frame to %d samples, the front end hops %d" % (hop_size(vocoder), cfg.hop_size))
        if vocoder.cin_channels != cfg.num_mels:
            raise ValueError("AudioInpainter: the vocoder takes %d conditioning channels, the front end makes %d mel bands"
                             % (vocoder.cin_channels, cfg.num_mels))
        self.model, self.vocoder, self.front = model, vocoder, front

    def __call__(self, wav, gap_start, gap_len, video=None, flow=None, uniforms=None, fade=0, return_parts=False):
        """wav (B, n) floats on the GPU, n a multiple of the hop, B one of 1, 2, 4, 8; gap_start / gap_len in SAMPLES of wav, one int or (B,) per
        stream, length 0 = no gap.  Returns the (B, n) waveform with each gap regenerated and every other sample copied bit for bit.

        The samples of the gap are silenced before anything reads them, the frames whose analysis window touches the gap are masked for the
        generator (`gap_frames`), and the vocoder is conditioned on the real mel outside those frames and on the generator's inside them.
        video / flow go to `model.set_inputs` (the visual branch); uniforms / fade to `inpaint_waveform` (the sampler's draws in window
        coordinates, the blend at the gap's end).
        `return_parts=True`: also a dict with `mask` (B, 1, 1, frames), `mel` (the damaged mel), `fake`, `c` (B, num_mels, frames), `aligned`
        (B, n + fft - hop) and `frames` (first, count per stream).

        The call OVERWRITES `model.mel`, `model.mask` and `model.fake` (and the embeddings `test()` leaves), as `set_inputs` + `test()` do; it runs
        the generator with `model.train = 0` (running BatchNorm statistics) and puts `model.train` back."""
        cfg = self.front.cfg
        fft, hop = int(cfg.fft_size), int(cfg.hop_size)
        if wav.dim() != 2:
            raise ValueError("AudioInpainter: wav is (B, n)")
        B, n = wav.shape
        if n < hop or n % hop != 0:
            raise ValueError("AudioInpainter: %d samples are not a whole number of %d-sample frames" % (n, hop))
        if B not in STREAM_COUNTS:
            raise ValueError("AudioInpainter: %d streams; a masked synthesis call runs the chain forms' 1, 2, 4 or 8" % B)
        if fade < 0:
            raise ValueError("AudioInpainter: fade >= 0")
        gs, gl = _per_stream(gap_start, B, "gap_start"), _per_stream(gap_len, B, "gap_len")
        if bool((gs < 0).any()) or bool((gl < 0).any()) or bool((gs + gl > n).any()):
            raise ValueError("AudioInpainter: a gap must lie inside the clip's %d samples" % n)
        l = fft - hop
        frames = self.front.num_frames(n)
        if frames * hop != n + l:
            raise ValueError("AudioInpainter: the front end makes %d frames of %d samples, the aligned clip has %d" % (frames, hop, n + l))
        why = generator_width_rule(frames, video.size(1) if getattr(self.model, "use_video", False) and video is not None else None)
        if why is not None:
            raise ValueError("AudioInpainter: " + why)
        if not wav.is_cuda:
            raise _lib.ViaiLibraryError("AudioInpainter runs on the GPU only; no CPU fallback")
        a0, a1 = gs + l, gs + l + gl
        a0_d, a1_d = _i32(a0, wav.device), _i32(a1, wav.device)
        aligned = wav_align(wav, a0_d, a1_d, l)
        mask = gap_frame_mask(a0_d, a1_d, frames, fft, hop)
        mel = self.front(aligned[:, l:], mask)
        model = self.model
        was = model.train
        model.train = 0
        try:
            model.set_inputs(mel, mask=mask, video=video, flow=flow)
            fake = model.test()
        finally:
            model.train = was
        c = mel_compose(mel, fake, mask)
        out = inpaint_waveform(self.vocoder, aligned, c, a0, gl, uniforms=uniforms, fade=fade, gap_unit="samples")[:, l:]
        if return_parts:
            return out, {"mask": mask, "mel": mel, "fake": fake, "c": c, "aligned": aligned, "frames": gap_frames(a0, a1, fft, hop, frames)}
        return out
