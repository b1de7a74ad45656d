"""viai_amd — MI355X-native hot path of the Vision-Infused Audio Inpainter (VIAI).

Import name: `viai_amd` (the on-disk directory keeps the project's hyphenated
name; the top-level `viai_amd/` shim maps the import name onto it).

  _lib      ctypes binding of libviai_hip.so (C ABI: include/viai_hip.h)
  ops       torch.autograd.Function wrappers (forward + backward in HIP)
  networks  MelEncoder / MelDecoder / MelDiscriminator shells (reference API + state_dict)
  model     AudioModel: the G+D train step (reference: the missing Models/Whole_Sync_inpainting_modify)
  ddp       one-process-per-GPU gradient all-reduce over RCCL
  synth     closed-form synthetic MUSICES-shaped inputs
  inpaint   AudioInpainter: waveform in, waveform out (mel front end -> generator -> WaveNet vocoder); gap_frames
  metrics   how good an inpainted clip is: gap SNR / SI-SDR, mel L1 / PSNR / log-spectral distance / SSIM, inpainting_report
  wav_resample  clips at any sample rate: Resampler (polyphase, HIP), gap_at_rate, inpaint_at_rate
  gap_detect    where a clip is damaged: find_gaps (dropouts, clipping, non-finite samples; HIP), find_gaps_host, repair
  ar_fill       short gaps without a network: Burg autoregressive interpolation, ar_fill (HIP), ar_fill_host, ar_fit_host
  janssen       dense runs (crackle) solved jointly per window: Janssen's least-squares AR interpolation, janssen_fill (HIP), janssen_fill_host,
                janssen_plan_host
  click_detect  where a clip holds clicks: find_clicks (outliers of an AR prediction residual; HIP), find_clicks_host, declick, declick_host,
                declick_file
  declip        clipped peaks restored under their bounds: declip_fill (bound-constrained Janssen; HIP), declip_fill_host, declip, declip_file
  video     raw frames and flow maps -> the visual branch's blocks: motion_box, resize_u8, prepare, VideoFrontEnd (HIP), motion_box_host
  optical_flow  raw frames -> TV-L1 flow -> the 8-bit flow maps `video` takes: tvl1, encode_u8, flow_u8 (HIP), tvl1_host, encode_u8_host
  wav_io    WAV in, WAV out: parse_wav, decode_pcm / encode_pcm / patch_pcm (HIP) and their _host mirrors, read_wav, write_wav, save_wav, repair_file
"""
__version__ = "0.1.0"


def __getattr__(name):
    # `viai_amd.AudioInpainter` / `viai_amd.gap_frames`, resolved on first use: importing the package stays free of torch and the library
    if name in ("AudioInpainter", "gap_frames"):
        from . import inpaint
        return getattr(inpaint, name)
    if name == "VideoFrontEnd":
        from . import video
        return video.VideoFrontEnd
    if name in ("tvl1", "encode_u8", "flow_u8", "tvl1_host", "encode_u8_host"):
        from . import optical_flow
        return getattr(optical_flow, name)
    if name in ("WavInfo", "parse_wav", "decode_pcm", "decode_pcm_host", "encode_pcm", "encode_pcm_host", "patch_pcm", "patch_pcm_host",
                "read_wav", "write_wav", "save_wav", "repair_file"):
        from . import wav_io
        return getattr(wav_io, name)
    if name in ("ar_fill_host", "ar_fit_host"):
        from . import ar_fill
        return getattr(ar_fill, name)
    if name in ("janssen_fill", "janssen_fill_host", "janssen_plan_host"):
        from . import janssen
        return getattr(janssen, name)
    if name in ("find_clicks", "find_clicks_host", "declick", "declick_host", "declick_file"):
        from . import click_detect
        return getattr(click_detect, name)
    if name in ("declip_fill", "declip_fill_host", "declip", "declip_file"):
        import importlib
        mod = importlib.import_module(".declip", __name__)                  # the module is callable: viai_amd.declip(wav, clip) is its declip()
        return mod if name == "declip" else getattr(mod, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
