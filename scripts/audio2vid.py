#!/usr/bin/env python3
"""audio2vid on MI355X — counterpart of the reference's scripts/audio2vid.py (:185-530) for the HIP path: BASELINE config 3,
"SMGA audio2pose + Stage-2 denoise".

    python scripts/audio2vid.py --synthetic -W 512 -H 512 -L 24 --steps 25
    python scripts/audio2vid.py --synthetic -L 24 --init_video clip.npy --regen_mask lips --paste_back    # dub an existing clip
    python scripts/audio2vid.py --synthetic --audio_path talk_48k.wav --audio_decoder device              # any PCM / float WAV, any rate

The chain is the reference's (line numbers of its scripts/audio2vid.py):
  1. Stage-1 SMGA (:198-200,324-348): one guided 50-step DDIM sample of 80 key-point frames per 3.2-second audio slice, each slice
     conditioned on frame 59 of the previous one (or on the reference image's pose), optional 5-candidate motion selection
     (`find_best_slice`, :79-108)                                  -> mmgt_amd.smga.SMGA.render_sample (HIP)
  2. seam smoothing by cubic splines around every 60th frame (:351-374)   -> host numpy / scipy, as in the reference
  3. key points -> pose / face / lips / hands frames (:386 `pose_vid_generator`: cv2 drawing of src/dwpose into four mp4 files, read
     back at :426-430) -> drawn on the device (mmgt_dwpose_draw, csrc/dwpose.hip: bit-exact on uint8 with oracle/dwpose_ref.py, the restatement of the
     reference drawers and of the OpenCV primitives under them; cv2 itself is not in this image, so that restatement is parity-unpinned), no files
  4. wav2vec2 features of the waveform (:420-426, src/dataset/audio_processor.py:76-131) -> mmgt_amd.wav2vec.Wav2VecModel (HIP);
     mask blur + 4-level pyramid (:453-476), audio window stack + AudioProjModel (:426,439-441) -> device kernels
  5. Pose2VideoPipeline (:484-498), frames converted to uint8 on the device, written as .npy / .gif / .avi / .apng / .png files / .webp.

--synthetic: random-init weights of the reference architectures (no checkpoints ship with the reference), a synthetic 16-kHz
waveform for the wav2vec2 leg, and synthetic WavLM + baseline features for SMGA (librosa extraction and vocal separation are host-side
and out of scope).  --wavlm {random,PATH} with --audio_path replaces the WavLM stand-in by real WavLM-Large features of the audio
(mmgt_amd.wavlm on HIP: the reference's slicing, scripts/audio2vid.py:299-315, and extract_wo_init); --baseline_feats supplies the 35
librosa columns.  Without --synthetic the script stops with a clear message: it would need those extractors, cv2 and PyAV.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("-c", "--config", default="./configs/prompts/animation.yaml")
    p.add_argument("--image_path", type=str)
    p.add_argument("--audio_path", type=str)
    p.add_argument("--decode_lossy_webp", action="store_true",
                   help="a .webp --image_path, lossy (VP8 key frames) or lossless, is decoded on the GPU (mmgt_amd.video_in.decode_webp_frames "
                        "with lossy=True, DESIGN 4n: PIL's bytes); without it, and for a file outside that decoder's scope (an alpha plane), "
                        "PIL opens the image on the host as before")
    p.add_argument("--decode_progressive_jpeg", action="store_true",
                   help="a .jpg / .jpeg --image_path, progressive (SOF2) or baseline, is decoded on the GPU (mmgt_amd.video_in.decode_jpeg_frames "
                        "with progressive=True, DESIGN 4o: libjpeg-turbo's bytes); without it, and for a file outside that decoder's scope, "
                        "PIL opens the image on the host as before")
    p.add_argument("--out_dir", type=str, default="scripts/output_videos")
    p.add_argument("--tem_dir", type=str, default="scripts/output_videos/temp")
    p.add_argument("-W", type=int, default=512)
    p.add_argument("-H", type=int, default=512)
    p.add_argument("-L", type=int, default=80)
    p.add_argument("--name", default="baseline_pose")
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--cfg", type=float, default=3.5)
    p.add_argument("--steps", type=int, default=30)
    p.add_argument("--fps", type=int)
    p.add_argument("--num_c", type=int, default=12, help="context frames per window")
    p.add_argument("--context_batch_size", type=int, default=1, help="context windows per UNet forward (the same sampler as 1)")
    p.add_argument("--use_motion_selection", default=False, action="store_true")
    p.add_argument("--num_epoch", type=int, default=3400)
    p.add_argument("--feature_type", type=str, default="wavlm")
    p.add_argument("--motion_diffusion_ckpt", type=str, default="./pretrained_weights/MMGT_pretrained/stage_1/audio2pose_best_model.pt")
    p.add_argument("--synthetic", action="store_true")
    p.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    p.add_argument("--format", default="npy", choices=["npy", "gif", "avi", "apng", "pngs", "webp"],
                   help="avi = Motion-JPEG encoded on the device, with the samples of --audio_path as its PCM sound track; apng = lossless animated "
                        "PNG, pngs = a directory of 0000.png, 0001.png, ..., both filtered and deflated on the device; webp = lossless animated "
                        "WebP, predicted and prefix-coded on the device (mmgt_amd.video_out)")
    p.add_argument("--quality", type=int, default=90, help="JPEG quality (1 .. 100) of --format avi")
    p.add_argument("--webp_quality", type=int, default=None,
                   help="with --format webp: 0 .. 100 writes lossy animated WebP, every frame a VP8 key frame coded on the device "
                        "(mmgt_amd.video_out.encode_vp8_frames); without it the .webp stays lossless")
    p.add_argument("--gif_encoder", default="pil", choices=["pil", "device"],
                   help="writer of --format gif: pil (per-frame palettes, on the host) or device (one palette for the clip, index map and LZW "
                        "on the device: mmgt_amd.video_out.encode_gif_frames)")
    p.add_argument("--gif_dither", default="none", choices=["none", "fs"],
                   help="with --gif_encoder device: fs = Floyd-Steinberg error diffusion against the clip's palette (smooth gradients stop banding; "
                        "the file grows)")
    p.add_argument("--gif_delta", action="store_true",
                   help="with --gif_encoder device: frame differencing, a pixel that keeps its palette index from one frame to the next is written "
                        "as the transparent index 255 (a palette of 255 colours)")
    p.add_argument("--audio_decoder", default="wave", choices=["wave", "device"],
                   help="reader of --audio_path: wave (stdlib, 16-kHz 16-bit PCM only) or device (mmgt_amd.audio_in, DESIGN 4r: any PCM / float "
                        "WAV, 8 .. 64 bits, 1 .. 16 channels, any rate, decoded, mixed down and resampled to 16 kHz on the GPU)")
    p.add_argument("--wavlm", default="off", metavar="{off,random,PATH}",
                   help="WavLM-Large features of --audio_path as columns 0:1024 of the SMGA conditioning: off (hash-seeded stand-in, the default), "
                        "random (hash-seeded Large weights) or the path of a WavLM-Large.pt checkpoint")
    p.add_argument("--baseline_feats", type=str, default=None,
                   help="(n_slices, 80, 35) .npy of the reference's librosa baseline features for columns 1024:1059 (librosa is not part of "
                        "this build; without it those columns keep the hash-seeded stand-in)")
    p.add_argument("--save_cond", type=str, default=None, help="write the (n_slices, 80, 1059) SMGA conditioning handed to the sampler to this .npy")
    p.add_argument("--sampler", default="ddim", choices=["ddim", "dpmpp2m"],
                   help="the update rule: the reference's DDIM, or DPM-Solver++ 2M (second order, the same one UNet forward per step; meant for fewer --steps)")
    p.add_argument("--eta", type=float, default=0.0, help="DDIM's stochasticity (0 = deterministic, 1 = ancestral); not with --sampler dpmpp2m")
    p.add_argument("--guidance_rescale", type=float, default=0.0,
                   help="in [0, 1]: rescale the guided prediction to the conditional one's standard deviation (Lin et al. 2305.08891, 3.4)")
    from mmgt_amd.longclip import add_longclip_arguments
    from mmgt_amd.inputs import add_revoice_arguments
    add_longclip_arguments(p)
    add_revoice_arguments(p)
    return p.parse_args()


def find_best_slice(slice_candidates, last_half):
    """scripts/audio2vid.py:79-108: the candidate whose first poses and mean velocity direction continue `last_half` best."""
    last_pos = last_half[-5:]
    last_v = np.mean((last_half[1:] - last_half[:-1])[-5:], axis=0).reshape(-1, 2)

    def v_angle_score(a, b):
        cos = np.sum(a * b, axis=1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
        return np.mean(np.arccos(np.clip(cos, -1.0, 1.0)))
    best, best_score = None, 1e9
    for cand in slice_candidates:
        cand_v = np.mean((cand[1:] - cand[:-1])[-5:], axis=0).reshape(-1, 2)
        score = np.sum(np.abs(cand[:5] - last_pos)) + v_angle_score(cand_v * 1000, last_v * 1000)
        if score < best_score:
            best, best_score = cand, score
    return best


def smooth_seams(tps_origin):
    """scripts/audio2vid.py:361-374: cubic-spline re-interpolation of 14 frames around every 60th frame."""
    from scipy.interpolate import CubicSpline
    out = tps_origin.copy()
    T = tps_origin.shape[0]
    for point in np.arange(60, T, 60):
        s, e = max(0, point - 5), min(T, point + 5)
        x = list(np.arange(s - 3, s)) + list(np.arange(e, e + 3))
        if min(x) < 0 or max(x) >= T:
            continue
        cs = CubicSpline(x, out[x], axis=0)
        out[s - 2:e + 2] = cs(np.arange(s - 2, e + 2))
    return out


def read_wav_16k(path):
    """Mono float waveform of a 16-kHz PCM .wav (stdlib `wave`; the reference resamples with librosa, which this build does not
    include: other rates are refused)."""
    import wave
    with wave.open(path, "rb") as w:
        if w.getframerate() != 16000:
            raise SystemExit(f"audio2vid: {path} is sampled at {w.getframerate()} Hz; resample to 16 kHz first (librosa is not part of this build), "
                             "or pass --audio_decoder device")
        if w.getsampwidth() != 2:
            raise SystemExit(f"audio2vid: {path} must be 16-bit PCM")
        pcm = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2").reshape(-1, w.getnchannels())
    return torch.from_numpy(pcm.astype(np.float32).mean(1) / 32768.0)


def read_wav_pcm(path, seconds):
    """The first `seconds` of a 16-bit PCM .wav as it is stored: (int16 samples (n, channels), sample rate) for write_avi's sound track."""
    import wave
    with wave.open(path, "rb") as w:
        if w.getsampwidth() != 2:
            raise SystemExit(f"audio2vid: {path} must be 16-bit PCM")
        n = min(w.getnframes(), int(round(seconds * w.getframerate())))
        return np.frombuffer(w.readframes(n), dtype="<i2").reshape(-1, w.getnchannels()), w.getframerate()


def main():
    a = parse_args()
    if not a.synthetic:
        raise SystemExit("non-synthetic runs need WavLM / librosa feature extraction, audio decoding, DWPose (onnxruntime, cv2) and PyAV, "
                         "which this build does not include; see INTEGRATION.md for wiring mmgt_amd into the reference's own script")
    if not torch.cuda.is_available():
        raise SystemExit("audio2vid needs an MI355X (the product has no CPU path)")
    from mmgt_amd import conditioning as C
    from mmgt_amd import hip
    from mmgt_amd.side_models import AudioProjModel
    from mmgt_amd.smga import SMGA
    from mmgt_amd.synthetic import build_synthetic_pipeline, hash_uniform, synth_state_dict, synth_tensor
    from mmgt_amd.video_out import save_videos_grid
    dev = torch.device("cuda:0")
    dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    timing = {}
    if a.audio_decoder == "device":                         # any PCM / float WAV: decode, down-mix and resampling on the device
        from mmgt_amd.audio_in import FORMAT_NAMES, parse_wav, pcm16_host, read_audio_device
        if not a.audio_path:
            raise SystemExit("audio2vid: --audio_decoder device goes with --audio_path")
        try:
            wav_info = parse_wav(a.audio_path)
        except ValueError as e:
            raise SystemExit(f"audio2vid: {e}")
        import functools
        read_wave = functools.lru_cache(None)(lambda path: read_audio_device(path, device=dev))      # both consumers share one decode; it stays on the device
        read_pcm = pcm16_host
    else:
        read_wave, read_pcm = read_wav_16k, read_wav_pcm
    t0 = time.time()
    from mmgt_amd.smga import smga_spec
    keys = smga_spec(cond_feature_dim=1059 if a.feature_type == "wavlm" else 35)
    smga_sd = {k: (synth_tensor("smga." + k, s) if not k.endswith("rotary.freqs") else torch.zeros(s)) for k, s in keys.items()}
    audio2pose = SMGA(feature_type=a.feature_type, device=dev, dtype=dtype, state_dict=smga_sd)             # :198-200
    pipe = build_synthetic_pipeline(dev, dtype)
    from mmgt_amd.scheduler import with_sampler
    pipe.scheduler = with_sampler(pipe.scheduler, a.sampler)
    audioproj = AudioProjModel(seq_len=5, blocks=12, channels=768, intermediate_dim=512, output_dim=768, context_tokens=32,
                               device=dev, dtype=dtype)                                                     # :264-273
    audioproj.load_state_dict(synth_state_dict(audioproj.spec, prefix="audioproj.", device=dev))
    timing["build_s"] = round(time.time() - t0, 2)

    # ---- 1. SMGA: audio -> key points, one 80-frame slice per 3.2 s (:300-348)
    n_slices = max(1, -(-a.L // 80))
    cond_list = hash_uniform("a2v.wavlm+baseline", (n_slices, 80, 1059), 1.0)          # WavLM (1024) + baseline (35) features per frame
    extra = {}
    if a.wavlm != "off":                                                                # :299-315: WavLM features of the audio slices
        from mmgt_amd.wavlm import WavLM, WavLMConfig, audio_slices, wavlm_spec
        if not a.audio_path:
            raise SystemExit("audio2vid: --wavlm needs --audio_path (a 16-kHz PCM .wav)")
        torch.cuda.synchronize()
        t0 = time.time()
        slices = audio_slices(read_wave(a.audio_path))
        if slices.shape[0] < n_slices or slices.shape[1] != 51200:
            raise SystemExit(f"audio2vid: {a.audio_path} gives {slices.shape[0]} slice(s) of {slices.shape[1]} samples; -L {a.L} needs "
                             f"{n_slices} full 3.2-s slices (the reference skips the first window of clips longer than 3.3 s)")
        if a.wavlm == "random":
            wavlm = WavLM(WavLMConfig(), device=dev, dtype=dtype)
            wavlm.load_state_dict(synth_state_dict(wavlm_spec(), prefix="wavlm.", device=dev))
        else:
            wavlm = WavLM.from_checkpoint(a.wavlm, device=dev, dtype=dtype)
        cond_list[:, :, :1024] = wavlm.slice_features(slices.to(dev)).cpu()[:n_slices]                  # all slices in one call
        del wavlm
        torch.cuda.synchronize()
        extra["wavlm"] = a.wavlm
        extra["wavlm_slices"] = int(slices.shape[0])
        extra["wavlm_s"] = round(time.time() - t0, 3)
        if a.baseline_feats:
            bf = torch.from_numpy(np.load(a.baseline_feats)).float()
            if tuple(bf.shape) != (n_slices, 80, 35):
                raise SystemExit(f"audio2vid: --baseline_feats holds {tuple(bf.shape)}, expected {(n_slices, 80, 35)}")
            cond_list[:, :, 1024:] = bf
        extra["baseline_feats"] = a.baseline_feats or "hash"
    elif a.baseline_feats:
        raise SystemExit("audio2vid: --baseline_feats goes with --wavlm random|PATH")
    if a.save_cond:
        np.save(a.save_cond, cond_list.numpy())
    init_feature = hash_uniform("a2v.init_pose", (1, 402), 0.8)                         # process_reference_image + mask_leg (:319-321)
    gen = torch.Generator(device=dev).manual_seed(a.seed)
    torch.cuda.synchronize()
    t0 = time.time()
    tps = []
    for i in range(n_slices):
        last_frame = init_feature if i == 0 else torch.from_numpy(tps[-1][59][None])                      # :327,333
        draw = lambda: audio2pose.render_sample(cond_frame=last_frame.float(), cond=cond_list[i], last_half=None, mode="normal",
                                                generator=gen).squeeze(0).cpu().numpy()
        if i > 0 and a.use_motion_selection:
            tps.append(find_best_slice([draw() for _ in range(5)], tps[-1]))                                # :334-342
        else:
            tps.append(draw())
    torch.cuda.synchronize()
    timing["smga_s"] = round(time.time() - t0, 3)
    tps_origin = np.concatenate([init_feature.numpy().astype(np.float32), np.concatenate(tps, 0)[:-1]], 0)  # :351-359
    kps = smooth_seams(tps_origin)[:a.L]                                                                     # (L, 402)

    # ---- 3. key points -> pose / face / lips frames: the reference's DWPose drawing (data/extract_movment_mask_all.py:319-321,
    # src/dwpose) on the device -- no mp4 files written and read back (:386,426-441)
    t0 = time.time()
    pose, face_u8, lips_u8, _hands_u8 = C.pose_frames_device(torch.from_numpy(kps).to(dev), a.H, a.W)
    # ---- 4. conditioning on the device (:426,439-441,453-476)
    face = C.mask_pyramid_device(C.blur_mask_device(face_u8, 31), a.H)
    lips = C.mask_pyramid_device(C.blur_mask_device(lips_u8, 21), a.H)
    full = C.full_mask_from_lips(lips)
    # wav2vec2 features of the (synthetic) 16-kHz waveform: AudioProcessor.preprocess (src/dataset/audio_processor.py:103-126) on the device
    from mmgt_amd.wav2vec import Wav2VecModel, wav2vec_spec
    w2v = Wav2VecModel(device=dev, dtype=dtype)
    w2v.load_state_dict(synth_state_dict(wav2vec_spec(), prefix="w2v.", device=dev))
    if a.audio_path:      # a 16-kHz PCM .wav drives the Stage-2 audio conditioning (audio_processor.py:103-110 loads with librosa at 16 kHz)
        wave = read_wave(a.audio_path)
        if a.audio_decoder == "device":
            extra["audio"] = {"rate": wav_info.rate, "channels": wav_info.channels, "fmt": FORMAT_NAMES[wav_info.fmt],
                              "samples_16k": int(wave.shape[0])}
        wave = wave[None, :a.L * 16000 // (a.fps or 25)]
    else:
        wave = hash_uniform("a2v.wave", (1, a.L * 16000 // (a.fps or 25)), 1.0)
    wave = ((wave - wave.mean()) / (wave.var(unbiased=False) + 1e-7).sqrt()).to(dev)                        # Wav2Vec2FeatureExtractor's normalisation
    feats = w2v.audio_emb(wave, a.L)                                                                        # (frames, 12 layers, 768)
    audio_tensor = audioproj(C.process_audio_emb_device(feats)[None])                                       # (1, L, 32, 768)
    torch.cuda.synchronize()
    timing["conditioning_s"] = round(time.time() - t0, 3)

    # ---- 5. Stage 2 (:484-498) + output path
    from PIL import Image
    ref_img = None
    if a.image_path and a.decode_lossy_webp and a.image_path.lower().endswith(".webp"):
        from mmgt_amd.video_in import decode_webp_frames
        try:
            with open(a.image_path, "rb") as fh:
                ref_img = Image.fromarray(decode_webp_frames([fh.read()], dev, limit=1, lossy=True)[0].cpu().numpy())
        except ValueError as e:                                  # outside the device decoder's scope: the parser says why
            print(f"note: {os.path.basename(a.image_path)} is decoded on the host ({e})")
    if a.image_path and a.decode_progressive_jpeg and a.image_path.lower().endswith((".jpg", ".jpeg")):
        from mmgt_amd.video_in import decode_jpeg_frames
        try:
            with open(a.image_path, "rb") as fh:
                ref_img = Image.fromarray(decode_jpeg_frames([fh.read()], dev, progressive=True)[0].cpu().numpy())
        except ValueError as e:                                  # outside the device decoder's scope: the parser says why
            print(f"note: {os.path.basename(a.image_path)} is decoded on the host ({e})")
    if ref_img is None and a.image_path:
        ref_img = Image.open(a.image_path).convert("RGB")
    elif ref_img is None:
        ref_img = Image.fromarray(((hash_uniform("a2v.ref", (a.H, a.W, 3), 0.5) + 0.5) * 255).clamp(0, 255).to(torch.uint8).numpy())
    # --init_video and its flags: the drawn 512 x 512 mask frames are the pixel masks (the pipeline resizes them to W x H)
    from mmgt_amd.longclip import longclip_kwargs
    from mmgt_amd.inputs import revoice_kwargs
    revoice = revoice_kwargs(a, {"face": face_u8, "lips": lips_u8, "hands": _hands_u8}, a.L, dev)
    t0 = time.time()
    out = pipe(ref_img, pose, audio_tensor.float(), full, face, lips, a.W, a.H, a.L, a.steps, a.cfg,
               generator=torch.manual_seed(a.seed), motion_scale=[1.0, 1.0, 2.0], context_frames=a.num_c,
               context_batch_size=a.context_batch_size, output_type="uint8", eta=a.eta, guidance_rescale=a.guidance_rescale,
               **longclip_kwargs(a), **revoice)
    torch.cuda.synchronize()
    timing["stage2_s"] = round(time.time() - t0, 3)
    v = torch.as_tensor(out.videos)                                                                          # (1, L, H, W, 3) uint8
    path = os.path.join(a.out_dir, f"audio2vid_synth_{a.W}x{a.H}x{a.L}.{a.format}")
    if a.format == "avi":                                  # JPEG on the device, the wav's own samples (the first L / fps seconds) as the sound track
        from mmgt_amd.video_out import encode_jpeg_frames, write_avi
        fps = a.fps or 25
        t0 = time.time()
        jpegs = encode_jpeg_frames(v[0], a.quality)
        sound = read_pcm(a.audio_path, a.L / fps) if a.audio_path else None
        extra["bytes"] = write_avi(path, jpegs, a.W, a.H, fps, audio=sound)
        extra["encode_s"] = round(time.time() - t0, 3)
    elif a.format == "pngs":                               # a directory that `ffmpeg -i %04d.png` reads
        from mmgt_amd.video_out import encode_png_frames, write_png_sequence
        path = os.path.splitext(path)[0] + "_png"
        extra["files"] = len(write_png_sequence(path, encode_png_frames(v[0]), a.W, a.H))
    else:
        lossy = a.webp_quality if a.format == "webp" else None
        gif = dict(gif_dither=None if a.gif_dither == "none" else a.gif_dither, gif_delta=a.gif_delta) if a.format == "gif" else {}
        save_videos_grid(v, path, n_rows=1, fps=a.fps or 25, gif_encoder=a.gif_encoder, webp_quality=lossy, **gif)
        if lossy is not None:
            extra["webp_quality"] = lossy
    print(json.dumps({"video": list(v.shape), "video_dtype": str(v.dtype), "saved": path, "slices": n_slices, "steps": a.steps,
                      "dtype": a.dtype, "context_batch_size": a.context_batch_size, "sampler": a.sampler, "eta": a.eta,
                      "guidance_rescale": a.guidance_rescale, "context_schedule": a.context_schedule, "context_fuse": a.context_fuse,
                      "guidance_interval": a.guidance_interval, "init_video": a.init_video, "strength": a.strength, "regen_mask": a.regen_mask,
                      "paste_back": a.paste_back, "keypoints_finite": bool(np.isfinite(kps).all()),
                      "mask_levels": [list(m.shape) for m in face], **timing, **extra}))


if __name__ == "__main__":
    main()
