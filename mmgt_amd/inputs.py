"""Caller-side inputs of the sampler from FILES (the callers either side of the hot path): the counterpart of
what `scripts/pose2vid.py:196-271` does between `read_frames(...)` and the pipeline call, with the per-frame mask arithmetic on the
device (mmgt_amd/conditioning.py) instead of cv2 / PIL on the host.

  read_frames        frames of a clip as PIL images (reference: src/utils/util.py read_frames, PyAV).  Containers that need a video
                     decoder (.mp4, .avi, .mov, .mkv, .webm) raise: PyAV / cv2 are not part of this build; a directory of images,
                     a .npy stack or an animated .gif / .png / .webp is read instead.  The one exception is an .avi whose video stream
                     is Motion-JPEG (what mmgt_amd.video_out.write_avi writes): its frames are JPEG files, which PIL decodes.
  pose_tensor        transforms.Resize((H, W)) + ToTensor of the pose frames -> (1, 3, L, H, W) float in [0, 1]
                     (scripts/pose2vid.py:231-236)
  motion_masks       face / lips / hands mask frames -> blur_mask (resize 64 x 64, Gaussian 31 / 21 / 21, min-max normalise) ->
                     the 64 / 32 / 16 / 8 pyramid -> full = clamp(1 - face + lips + hands, 0, 1) per level (:239-271)
  pose_tensor_device / motion_masks_device
                     the same two from uint8 RGB frames that are already on the device (mmgt_amd.video_in.read_frames_device: Motion-JPEG
                     decoded there): no PIL, no host copy of a frame.  pose_tensor_device(resize=True) takes frames of any size:
                     PIL's antialiased bilinear resize runs on the device, byte for byte
  resize_frames_device / ref_image_tensors_device
                     PIL's Image.resize (bilinear / bicubic / Lanczos) on device frames, and the reference image's two prologue inputs
                     (the VAE's Lanczos-resized [-1, 1] tensor, CLIP's bicubic 224 x 224 normalised pixel values) from a device image
  add_revoice_arguments / revoice_kwargs
                     the scripts' flags of re-voicing an existing clip (--init_video, --strength, --regen_mask, --mask_grow, --paste_back,
                     --feather) and the pipeline arguments they become
  load_checkpoint    a state dict from .safetensors / .pth / .pt / .bin / .ckpt or a diffusers-style directory
  split_net_checkpoint   the reference's `Net` checkpoint (net-<num_c>.pth, scripts/pose2vid.py:41-67,186-190) -> per-module dicts
"""
import os
from pathlib import Path
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

VIDEO_CONTAINERS = {".mp4", ".avi", ".mov", ".mkv", ".webm", ".m4v"}
IMAGE_SUFFIXES = {".png", ".jpg", ".jpeg", ".bmp", ".webp", ".tif", ".tiff"}


def _riff_chunks(buf, start, end):
    """(fourcc, body offset, body size) of the chunks in buf[start:end]; chunks are padded to even length."""
    pos = start
    while pos + 8 <= end:
        size = int.from_bytes(buf[pos + 4:pos + 8], "little")
        yield buf[pos:pos + 4], pos + 8, size
        pos += 8 + size + (size & 1)


def mjpeg_avi_frames(path, limit: Optional[int] = None):
    """The JPEG files of the '00dc' chunks of a RIFF AVI whose first video stream is MJPG, in file order; None if `path` is not such a file
    (another container, another codec)."""
    with open(path, "rb") as fh:
        buf = fh.read()
    if len(buf) < 12 or buf[:4] != b"RIFF" or buf[8:12] != b"AVI ":
        return None
    codec, frames = None, []
    for cc, off, size in _riff_chunks(buf, 12, len(buf)):
        if cc != b"LIST":
            continue
        kind = buf[off:off + 4]
        if kind == b"hdrl":
            for cc2, off2, size2 in _riff_chunks(buf, off + 4, off + size):
                if cc2 == b"LIST" and buf[off2:off2 + 4] == b"strl" and codec is None:
                    for cc3, off3, size3 in _riff_chunks(buf, off2 + 4, off2 + size2):
                        if cc3 == b"strh" and buf[off3:off3 + 4] == b"vids":
                            codec = buf[off3 + 4:off3 + 8]
        elif kind == b"movi":
            if codec is None or codec.upper() != b"MJPG":
                return None
            for cc2, off2, size2 in _riff_chunks(buf, off + 4, off + size):
                if cc2 == b"00dc" and (limit is None or len(frames) < limit):
                    frames.append(buf[off2:off2 + size2])
    return frames if codec is not None and codec.upper() == b"MJPG" else None


def read_frames(path, limit: Optional[int] = None) -> list:
    """PIL frames of `path`: a directory of images (sorted by name), a .npy stack (L, H, W[, C]) uint8, an animated image
    (.gif / .png / .webp), one still image, or a Motion-JPEG .avi."""
    from PIL import Image, ImageSequence
    p = Path(path)
    if not p.exists():
        raise FileNotFoundError(f"read_frames: {p} does not exist")
    if p.is_dir():
        files = sorted(f for f in p.iterdir() if f.is_file() and f.suffix.lower() in IMAGE_SUFFIXES)
        if not files:
            raise RuntimeError(f"read_frames: no image files ({', '.join(sorted(IMAGE_SUFFIXES))}) in {p}")
        return [Image.open(f).copy() for f in (files if limit is None else files[:limit])]
    suf = p.suffix.lower()
    if suf == ".avi":
        import io
        jpegs = mjpeg_avi_frames(p, limit)
        if jpegs is not None:
            return [Image.open(io.BytesIO(j)).convert("RGB") for j in jpegs]
    if suf in VIDEO_CONTAINERS:
        raise RuntimeError(f"read_frames: {p.name} needs a video decoder (PyAV / cv2: src/utils/util.py read_frames), which this build "
                           f"does not include -- extract the frames into a directory of images or a .npy stack and pass that instead")
    if suf == ".npy":
        arr = np.load(p)
        if arr.dtype != np.uint8 or arr.ndim not in (3, 4):
            raise RuntimeError(f"read_frames: {p.name} must hold uint8 frames (L, H, W) or (L, H, W, C), got {arr.dtype} {arr.shape}")
        arr = arr if limit is None else arr[:limit]
        return [Image.fromarray(f) for f in arr]
    img = Image.open(p)
    frames = [f.copy() for f in ImageSequence.Iterator(img)]
    return frames if limit is None else frames[:limit]


def pose_tensor(frames: Sequence, width: int, height: int) -> torch.Tensor:
    """(1, 3, L, H, W) float32 in [0, 1]: torchvision's Resize((H, W)) (PIL bilinear with antialias) + ToTensor per frame."""
    from PIL import Image
    out = []
    for f in frames:
        f = f.convert("RGB")
        if f.size != (width, height):
            f = f.resize((width, height), Image.BILINEAR)
        out.append(torch.from_numpy(np.asarray(f, dtype=np.uint8).copy()))
    x = torch.stack(out).permute(3, 0, 1, 2).float().div_(255.0)      # (3, L, H, W)
    return x.unsqueeze(0)


def _mask_stack(frames: Sequence, length: int) -> torch.Tensor:
    """Mask frames -> (L, h, w) uint8 (single channel: the reference blurs the array as read and converts to "L" afterwards; mask
    videos are grey, so the first channel is the mask)."""
    arrs = []
    for f in frames[:length]:
        a = np.asarray(f)
        arrs.append(torch.from_numpy((a if a.ndim == 2 else a[..., 0]).astype(np.uint8).copy()))
    return torch.stack(arrs)


def motion_masks(face_frames: Sequence, lips_frames: Sequence, hands_frames: Optional[Sequence], length: int, device,
                 img_size: int = 512):
    """-> (full, face, lips): three lists of four (L, (64 / 2^k)^2) float tensors on the CPU, as the pipeline takes them."""
    from . import conditioning as C

    def pyramid(frames, ksize):
        u8 = _mask_stack(frames, length).to(device).contiguous()
        return [m.cpu() for m in C.mask_pyramid_device(C.blur_mask_device(u8, ksize), img_size)]
    face = pyramid(face_frames, 31)
    lips = pyramid(lips_frames, 21)
    if hands_frames is not None:
        hands = pyramid(hands_frames, 21)
    else:
        hands = [torch.zeros_like(m) for m in lips]                   # `Image.new("L", (64, 64), 0)` (:252)
    return C.full_mask_with_hands(face, lips, hands), face, lips


_RESAMPLE = ("bilinear", "bicubic", "lanczos")
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)                      # CLIPImageProcessor's image_mean / image_std
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def _check_frames(x, what, channels=(3,)):
    if not isinstance(x, torch.Tensor) or x.dtype != torch.uint8 or x.dim() != 4 or x.shape[3] not in channels:
        raise ValueError(f"{what}: expected uint8 (L, H, W, {' or '.join(map(str, channels))}) frames, got {getattr(x, 'dtype', type(x))} "
                         f"{tuple(getattr(x, 'shape', ()))}")


def resize_frames_device(frames_u8: torch.Tensor, width: int, height: int, resample: str = "bilinear") -> torch.Tensor:
    """(L, h, w, C) uint8 frames on the device, C = 1 or 3 -> (L, height, width, C) uint8 there: PIL's Image.resize((width, height), resample) of
    every frame, byte for byte.  resample: "bilinear" (transforms.Resize), "bicubic" (Image.resize's default) or "lanczos"."""
    from . import conditioning as C
    _check_frames(frames_u8, "resize_frames_device", (1, 3))
    if resample not in _RESAMPLE:
        raise ValueError(f"resize_frames_device: resample {resample!r} is not one of {_RESAMPLE}")
    if not frames_u8.is_cuda:
        raise ValueError("resize_frames_device: the frames must be on the device")
    return C.resize_u8_device(frames_u8.contiguous(), height, width, resample)


def pose_tensor_device(frames_u8: torch.Tensor, width: int, height: int, resize: bool = False) -> torch.Tensor:
    """(L, h, w, 3) uint8 RGB on the device -> (1, 3, L, H, W) float32 in [0, 1] there: pose_tensor's u8 / 255 in fp32, exactly.  Frames of another
    size raise unless resize=True, which runs pose_tensor's antialiased bilinear resize (PIL's, byte for byte) on the device first."""
    from . import conditioning as C
    x = frames_u8
    _check_frames(x, "pose_tensor_device")
    if tuple(x.shape[1:3]) != (height, width) and not resize:
        raise ValueError(f"pose_tensor_device: the frames are {x.shape[2]} x {x.shape[1]}, the sampler wants {width} x {height}; pass resize=True for "
                         "the antialiased resize on the device, or use read_frames + pose_tensor")
    # the 256 quotients come from the host, where pose_tensor divides: a device division by a scalar multiplies by the rounded reciprocal instead
    lut = (torch.arange(256, dtype=torch.float32) / 255.0).repeat(3, 1).to(x.device)
    return C.resize_u8_device(x.contiguous(), height, width, "bilinear", lut=lut)[None]


def ref_image_tensors_device(ref_u8: torch.Tensor, width: int, height: int):
    """The two prologue inputs of the sampler from ONE reference image (h, w, 3) uint8 RGB on the device ->
      vae_input   (1, 3, height, width) float32 in [-1, 1]: Lanczos resize, u8 / 255 * 2 - 1 -- pipeline._pil_to_tensor(img, width, height, True), exactly;
      clip_pixels (1, 3, 224, 224) float32: bicubic resize to 224 x 224 (PIL's default filter), then (v / 255 - mean_c) / std_c with CLIP's mean
                  and std -- CLIPImageProcessor's rescale and normalize in its order of float32 operations.
    Both float stages are 256-entry tables computed on the host with the host route's own operations; the device only looks them up."""
    from . import conditioning as C
    x = ref_u8
    if not isinstance(x, torch.Tensor) or x.dtype != torch.uint8 or x.dim() != 3 or x.shape[2] != 3 or not x.is_cuda:
        raise ValueError(f"ref_image_tensors_device: expected a uint8 (h, w, 3) image on the device, got {getattr(x, 'dtype', type(x))} "
                         f"{tuple(getattr(x, 'shape', ()))}")
    x = x.contiguous()[None]
    v = np.arange(256)
    vae_lut = torch.from_numpy(v.astype(np.float32) / 255.0) * 2.0 - 1.0                       # _pil_to_tensor's operations
    unit = (v.astype(np.float64) * (1 / 255)).astype(np.float32)                               # the processor rescales in float64, then float32
    clip_lut = np.stack([(unit - np.float32(m)) / np.float32(s) for m, s in zip(CLIP_MEAN, CLIP_STD)])
    vae_in = C.resize_u8_device(x, height, width, "lanczos", lut=vae_lut.repeat(3, 1).to(x.device))
    clip_in = C.resize_u8_device(x, 224, 224, "bicubic", lut=torch.from_numpy(clip_lut).to(x.device))
    return vae_in.permute(1, 0, 2, 3), clip_in.permute(1, 0, 2, 3)                              # n = 1: the same memory as (1, 3, H, W)


def motion_masks_device(face_u8: torch.Tensor, lips_u8: torch.Tensor, hands_u8: Optional[torch.Tensor], length: int, img_size: int = 512):
    """motion_masks for (L, h, w, 3) uint8 RGB mask frames that are already on the device: channel 0 is the mask (as in _mask_stack), and blur and
    pyramid run where the frames are.  -> (full, face, lips) as motion_masks returns them."""
    from . import conditioning as C

    def pyramid(frames, ksize, name):
        if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or frames.dim() != 4 or not frames.is_cuda:
            raise ValueError(f"motion_masks_device: {name} must be uint8 (L, h, w, 3) frames on the device")
        u8 = frames[:length, :, :, 0].contiguous()
        return [m.cpu() for m in C.mask_pyramid_device(C.blur_mask_device(u8, ksize), img_size)]
    face = pyramid(face_u8, 31, "face")
    lips = pyramid(lips_u8, 21, "lips")
    hands = pyramid(hands_u8, 21, "hands") if hands_u8 is not None else [torch.zeros_like(m) for m in lips]
    return C.full_mask_with_hands(face, lips, hands), face, lips


def add_revoice_arguments(p):
    """The flags of re-voicing an existing clip, shared by scripts/pose2vid.py and scripts/audio2vid.py."""
    p.add_argument("--init_video", type=str, default=None,
                   help="an existing clip to re-voice instead of sampling from noise: anything read_frames reads (a directory of images, .npy, "
                        "Motion-JPEG .avi, .apng, .gif, .webp); frames of another size are Lanczos-resized on the device")
    p.add_argument("--strength", type=float, default=1.0,
                   help="with --init_video: the part of the schedule that is run, in (0, 1]: the last int(steps * strength) steps")
    p.add_argument("--regen_mask", type=str, default=None,
                   help="with --init_video: the region that is re-synthesised -- face, lips or full (face + lips + hands) of the run's own mask "
                        "clips, or the path of a mask clip (>= 128 = regenerate); the rest of the clip is kept")
    p.add_argument("--mask_grow", type=int, default=1, help="latent cells (8 x 8 pixels) by which --regen_mask is dilated, 0 .. 8")
    p.add_argument("--paste_back", action="store_true",
                   help="with --init_video: composite the decoded frames onto the clip's own frames outside the (feathered) mask, on the device")
    p.add_argument("--feather", type=int, default=8, help="radius in pixels of the box blur of --paste_back's alpha, 0 .. 32")


def frames_tensor_u8(frames: Sequence) -> torch.Tensor:
    """PIL frames of one size -> (L, h, w, 3) uint8 RGB"""
    arrs = [np.asarray(f.convert("RGB"), dtype=np.uint8) for f in frames]
    if len({a.shape for a in arrs}) != 1:
        raise RuntimeError(f"the frames of a clip must have one size, got {sorted({a.shape[:2] for a in arrs})}")
    return torch.from_numpy(np.stack(arrs))


def revoice_kwargs(a, masks: Dict[str, Optional[torch.Tensor]], length: int, device, on_device: bool = False, **decode_kw) -> dict:
    """The pipeline's init arguments from the flags of `add_revoice_arguments`.  masks: {"face", "lips", "hands"} -> (L, h, w) uint8 pixel masks
    (tensor or None) of the run's own mask clips, for --regen_mask face / lips / full.  The clip is read on the device when on_device and its
    container is one read_frames_device takes (everything but .npy); the flags without --init_video are handed on, and the pipeline refuses them."""
    kw = {}
    if a.strength != 1.0:
        kw["strength"] = a.strength
    if a.paste_back:
        kw["paste_back"] = True
    if a.init_video:
        if on_device and not str(a.init_video).lower().endswith(".npy"):
            from .video_in import read_frames_device
            clip = read_frames_device(a.init_video, length, device, **decode_kw)
        else:
            clip = frames_tensor_u8(read_frames(a.init_video, length)).to(device)
        if clip.shape[0] < length:
            raise SystemExit(f"--init_video {a.init_video} has {clip.shape[0]} frames, the run samples {length}")
        kw.update(init_video=clip[:length].contiguous(), mask_grow=a.mask_grow, feather=a.feather)
    if a.regen_mask:
        if a.regen_mask in ("face", "lips", "full"):
            names = ("face", "lips", "hands") if a.regen_mask == "full" else (a.regen_mask,)
            parts = [masks[n][:length].to(device) for n in names if masks.get(n) is not None]
            if not parts or len({tuple(p.shape) for p in parts}) != 1:
                raise SystemExit(f"--regen_mask {a.regen_mask}: the run's mask clips are missing or differ in size")
            m = parts[0]
            for q in parts[1:]:
                m = torch.maximum(m, q)
        else:
            m = _mask_stack(read_frames(a.regen_mask, length), length).to(device)
        kw["regen_mask"] = m.contiguous()
    return kw


def load_checkpoint(path) -> Dict[str, torch.Tensor]:
    """State dict of a checkpoint file, or of a diffusers / transformers-style directory (first of diffusion_pytorch_model.safetensors,
    model.safetensors, diffusion_pytorch_model.bin, pytorch_model.bin)."""
    p = Path(path)
    if p.is_dir():
        for name in ("diffusion_pytorch_model.safetensors", "model.safetensors", "diffusion_pytorch_model.bin", "pytorch_model.bin"):
            if (p / name).is_file():
                p = p / name
                break
        else:
            raise FileNotFoundError(f"load_checkpoint: no weights file found in {p}")
    if not p.is_file():
        raise FileNotFoundError(f"load_checkpoint: {p} does not exist")
    if p.suffix == ".safetensors":
        from safetensors.torch import load_file
        return load_file(str(p), device="cpu")
    if p.suffix in (".pth", ".pt", ".bin", ".ckpt"):
        sd = torch.load(str(p), map_location="cpu", weights_only=True)
        return sd.get("state_dict", sd) if isinstance(sd, dict) else sd
    raise RuntimeError(f"load_checkpoint: unknown file format {p.suffix!r} ({p})")


NET_PREFIXES = ("reference_unet", "denoising_unet", "pose_guider", "audioproj")


def split_net_checkpoint(sd: Dict[str, torch.Tensor]) -> Dict[str, Dict[str, torch.Tensor]]:
    """The reference trains and stores its modules as one `Net` (scripts/pose2vid.py:41-67): keys `<module>.<key>`."""
    out = {p: {} for p in NET_PREFIXES}
    for k, v in sd.items():
        head, _, rest = k.partition(".")
        if head not in out:
            raise RuntimeError(f"split_net_checkpoint: unexpected key {k!r} (expected one of {NET_PREFIXES} as the first component)")
        out[head][rest] = v
    return out
