"""mmgt_amd: MI355X-native Stage-2 denoising path of MMGT (UNet3D + MM-HAA, DDIM loop, VAE decode).

The arithmetic lives in hand-written HIP kernels (mmgt_amd/csrc, built into libmmgt_hip.so and reached through the
C ABI declared in include/mmgt_hip.h); the Python here mirrors the reference's operator interface
(src/models/unet_3d.py, src/pipelines/pipeline_pose2vid_long.py) and does plumbing only.
"""
__version__ = "0.1.0"


def __getattr__(name):
    # WavLM / WavLMConfig are exported lazily: `import mmgt_amd` stays as light as it was, and only a caller that asks for them
    # imports mmgt_amd.wavlm (and torch) -- `from mmgt_amd import WavLM` works as for any other export
    if name in ("WavLM", "WavLMConfig"):
        from . import wavlm
        return getattr(wavlm, name)
    if name in ("parse_jpeg", "decode_jpeg_frames", "parse_png", "decode_png_frames", "parse_gif", "decode_gif_frames",
                "parse_webp", "decode_webp_frames", "read_frames_device"):
        from . import video_in
        return getattr(video_in, name)
    if name in ("pose_tensor_device", "motion_masks_device", "resize_frames_device", "ref_image_tensors_device"):
        from . import inputs
        return getattr(inputs, name)
    if name in ("parse_wav", "WavInfo", "resample_plan", "resample_device", "read_audio_device"):
        from . import audio_in
        return getattr(audio_in, name)
    raise AttributeError(f"module 'mmgt_amd' has no attribute {name!r}")
