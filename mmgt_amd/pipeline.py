"""Pose2VideoPipeline on MI355X: windowed DDIM sampling around the HIP denoise-step operator.

Host-side mirror of src/pipelines/pipeline_pose2vid_long.py:35-660 (used by scripts/pose2vid.py and scripts/audio2vid.py)
and of the single-window src/pipelines/pipeline_pose2vid.py:284-506 (= context_frames >= video_length).  Same constructor
and __call__ signature; the per-step tensor arithmetic (window accumulate, overlap average, CFG combine, DDIM update) runs
in two HIP kernels on fp32 latents that never leave the GPU.

Extensions through **kwargs (allowed by the reference signature, :365): `latents=` (inject initial noise, parity tests),
`clip_image_embeds=` / `ref_image_latents=` / `reference_banks=` / `pose_features=` (hand over prologue results when the module
is None), `decode=False`, `window_group=` / `cfg_split=` (window-parallel sampling of one long video over several GPUs).
`context_batch_size=B` runs the window loop B windows per forward: the same sampler as B = 1 (see `denoise`).
`eta` (the reference's extra_step_kwargs), `guidance_rescale=` (rescale_noise_cfg of pipeline_lmks2vid_long.py) and a
`DPMSolverMultistepScheduler` as `scheduler` select the update behind the accumulation (see `denoise`); the defaults are the reference's DDIM.
`ref_image` may be a uint8 (h, w, 3) RGB tensor instead of a PIL image: the Lanczos resize in front of the VAE and the bicubic 224 x 224 resize
in front of CLIP then run on the device (mmgt_amd.inputs.ref_image_tensors_device), with PIL's bytes.
`init_video=` / `init_latents=`, `strength=`, `regen_mask=`, `mask_grow=`, `paste_back=`, `feather=` re-voice an existing clip instead of sampling
from noise: the clip is noised to the start of the last int(N strength) steps, the cells outside the mask are put back after every
step, and the decoded frames can be composited onto the clip's own frames on the device.
`output_type="uint8"` returns the frames as uint8 (b, f, H, W, 3), converted on the device (what save_videos_grid writes).
`output_type="jpeg"` (with `jpeg_quality=`, `jpeg_subsampling=`) returns one JPEG file (bytes) per frame, encoded on the device.
"""
import math
from dataclasses import dataclass, field
from typing import Callable, List, Optional, Union

import numpy as np

import torch

from . import hip, parallel
from .longclip import get_context_scheduler


@dataclass
class Pose2VideoPipelineOutput:
    videos: Union[torch.Tensor, np.ndarray]


@dataclass
class _Unit:
    """One forward of the sampler loop: 1 to B windows of the clip's window list, for the CFG pair (`row` None; batch rows in CFG row major order
    [uncond w0 .. uncond w(n-1), cond w0 .. cond w(n-1)]) or for one CFG row alone (`row` 0 or 1), with its step-invariant conditioning and the memo
    (`state`) in which the HIP operator keeps what it derives from exactly these rows."""
    windows: List[int]                    # numbers in the window list
    row: Optional[int]
    long: torch.Tensor                    # (n, Fw) long: the windows' frames, for the gather from the latents
    idx: torch.Tensor                     # the same in int32, in the shape the accumulate entry takes: (Fw,) at context_batch_size 1, else (n, Fw)
    pose: Optional[torch.Tensor]
    audio: torch.Tensor
    full: List[torch.Tensor]
    face: List[torch.Tensor]
    lips: List[torch.Tensor]
    state: dict = field(default_factory=dict)
    halves: dict = field(default_factory=dict)

    def half(self, row):
        """The unit of CFG row `row` of this pair, cut on first use: every tensor of a pair is [row 0 | row 1] along its first axis.  The memo is a
        dict of its own (the pair's holds rows of another shape)."""
        if row not in self.halves:
            cut = lambda t: t.view(2, t.shape[0] // 2, *t.shape[1:])[row].contiguous()
            self.halves[row] = _Unit(self.windows, row, self.long, self.idx, None if self.pose is None else cut(self.pose), cut(self.audio),
                                   [cut(m) for m in self.full], [cut(m) for m in self.face], [cut(m) for m in self.lips])
        return self.halves[row]


def _pil_to_tensor(img, width, height, normalize):
    """VaeImageProcessor.preprocess for one PIL image: RGB, lanczos resize, /255, CHW, optional 2x-1 (App. B-6)."""
    from PIL import Image
    img = img.convert("RGB").resize((width, height), resample=Image.LANCZOS)
    arr = torch.from_numpy(np.asarray(img).astype(np.float32) / 255.0).permute(2, 0, 1)
    return arr * 2.0 - 1.0 if normalize else arr


class Pose2VideoPipeline:
    def __init__(self, vae, image_encoder, reference_unet, denoising_unet, pose_guider, scheduler,
                 image_proj_model=None, tokenizer=None, text_encoder=None):
        self.vae = vae
        self.image_encoder = image_encoder
        self.reference_unet = reference_unet
        self.denoising_unet = denoising_unet
        self.pose_guider = pose_guider
        self.scheduler = scheduler
        self.image_proj_model = image_proj_model
        self.tokenizer = tokenizer
        self.text_encoder = text_encoder
        self.vae_scale_factor = 8          # 2 ** (len(vae.config.block_out_channels) - 1) for sd-vae-ft-mse

    def to(self, device=None, dtype=None):
        return self

    @property
    def device(self):
        return self.denoising_unet.device

    # --------------------------------------------------------------------------------------------- helpers
    def prepare_latents(self, batch_size, num_channels_latents, width, height, video_length, dtype, device, generator,
                        latents=None):
        """pipeline_pose2vid_long.py:148-182; noise is drawn on the generator's device then moved (App. B-7)."""
        shape = (batch_size, num_channels_latents, video_length, height // self.vae_scale_factor,
                 width // self.vae_scale_factor)
        if isinstance(generator, list) and len(generator) != batch_size:
            raise ValueError(
                f"You have passed a list of generators of length {len(generator)}, but requested an effective batch"
                f" size of {batch_size}. Make sure the batch size matches the length of the generators.")
        if latents is None:
            gdev = generator.device if isinstance(generator, torch.Generator) else torch.device("cpu")
            latents = torch.randn(shape, generator=generator if isinstance(generator, torch.Generator) else None,
                                  device=gdev, dtype=torch.float32)
        latents = latents.to(device=device, dtype=torch.float32)
        return (latents * self.scheduler.init_noise_sigma).contiguous()

    def decode_latents(self, latents, window_group=None, uint8=False):
        """pipeline_pose2vid_long.py:112-125: frame-by-frame VAE decode of z / 0.18215, (x/2+0.5).clamp(0,1), fp32 CPU.
        With a window_group the frames (independent units) are dealt in contiguous runs to the ranks and all-gathered, so
        every rank returns the whole video ("VAE decode sharded by frame")."""
        if self.vae is None:
            raise RuntimeError("decode_latents needs a VAE (pass decode=False to get latents)")
        if window_group is None and uint8:
            return self.vae.decode_video_uint8(latents).cpu().numpy()      # (b, f, H, W, 3) uint8: save_videos_grid's frames
        if window_group is None:
            video = self.vae.decode_video(latents)           # (b, 3, f, H, W) fp32 in [0, 1] on the GPU
            return video.cpu().float().numpy()
        group = None if window_group is True else window_group
        world, rank = parallel.dist.get_world_size(group), parallel.dist.get_rank(group)
        f = latents.shape[2]
        per = (f + world - 1) // world                       # equal runs (the last ranks repeat the final frame as padding)
        idx = torch.arange(rank * per, (rank + 1) * per, device=latents.device).clamp_(max=f - 1)
        if uint8:                                            # (b, per, H, W, 3) uint8 per rank: a quarter of the fp32 bytes on the wire
            part = self.vae.decode_video_uint8(latents[:, :, idx])
            parts = parallel.allgather_window_predictions(part, group)
            return torch.cat(parts, dim=1)[:, :f].cpu().numpy()
        part = self.vae.decode_video(latents[:, :, idx])
        parts = parallel.allgather_window_predictions(part, group)
        return torch.cat(parts, dim=2)[:, :, :f].cpu().float().numpy()

    def decode_latents_jpeg(self, latents, window_group=None, quality=90, subsampling="4:2:0"):
        """The frames of ONE clip as JPEG files (AutoencoderKL.decode_video_jpeg): a list of f byte strings.  With a window_group each rank
        decodes and encodes its own contiguous run of frames and the byte strings are gathered, so every rank returns the whole list."""
        if self.vae is None:
            raise RuntimeError("decode_latents needs a VAE (pass decode=False to get latents)")
        if latents.shape[0] != 1:
            raise ValueError(f'output_type="jpeg" returns one list of frames: batch 1 only, got batch {latents.shape[0]}')
        if window_group is None:
            return self.vae.decode_video_jpeg(latents, quality, subsampling)
        group = None if window_group is True else window_group
        world, rank = parallel.dist.get_world_size(group), parallel.dist.get_rank(group)
        f = latents.shape[2]
        per = (f + world - 1) // world
        lo, hi = min(rank * per, f), min((rank + 1) * per, f)
        mine = self.vae.decode_video_jpeg(latents[:, :, lo:hi], quality, subsampling) if hi > lo else []
        parts = [None] * world
        parallel.dist.all_gather_object(parts, mine, group=group)
        return [j for part in parts for j in part]

    def interpolate_latents(self, latents, interpolation_factor, device=None):
        """pipeline_pose2vid_long.py:292-335 (no-op below factor 2): all pairs and rates in one batched expression."""
        from .interp import interpolate_frames
        return interpolate_frames(latents, interpolation_factor)

    def _pose_group(self, pose_fea, cs):
        """Pose features of the windows `cs` for both CFG rows (pipeline_pose2vid_long.py:576-580), CFG row major [w0 .. w(B-1), w0 .. w(B-1)],
        converted ONCE to the operator's channels-last layout and dtype: they are step-invariant, so the per-step forward takes them as is."""
        if pose_fea is None:
            return None
        unet = self.denoising_unet
        p5 = torch.cat([pose_fea[:, :, c] for c in cs]).repeat(2, 1, 1, 1, 1).to(torch.float32).contiguous()
        if not p5.is_cuda or not hasattr(unet, "boc"):
            return p5
        return hip.ncfhw_to_nhwc(p5, p5.shape[1], unet.dtype)

    def _check_update_args(self, eta, guidance_rescale, window_group):
        """The refusals of the update's arguments (each names both parties); -> whether the scheduler is the multistep solver."""
        from .scheduler import DPMSolverMultistepScheduler
        dpm = isinstance(self.scheduler, DPMSolverMultistepScheduler)
        if eta < 0.0:
            raise ValueError(f"eta must not be negative, got eta={eta}")
        if eta > 0.0 and dpm:
            raise ValueError(f"eta={eta} is not combined with scheduler=DPMSolverMultistepScheduler (DPM-Solver++ 2M is deterministic): use "
                             "eta=0 or a DDIMScheduler")
        if eta > 0.0 and window_group is not None:
            raise ValueError(f"eta={eta} is not combined with window_group (every rank would draw its own noise and the latents would part): "
                             "use eta=0 or one GPU")
        if not 0.0 <= guidance_rescale <= 1.0:
            raise ValueError(f"guidance_rescale must lie in [0, 1] (it blends the rescaled guidance_scale prediction with the plain one), got "
                             f"guidance_rescale={guidance_rescale}")
        return dpm

    def _check_loop_args(self, eta, guidance_rescale, window_group, context_fuse, guidance_interval, context_batch_size):
        """The refusals of the loop's options, for `__call__` (before any model is touched) and `denoise` alike
        -> (eta, guidance_rescale, whether the scheduler is the multistep solver, the checked interval, B)."""
        from .longclip import CONTEXT_FUSES, check_guidance_interval
        if context_fuse not in CONTEXT_FUSES:
            raise ValueError(f"context_fuse must be one of {', '.join(CONTEXT_FUSES)}, got context_fuse={context_fuse!r}")
        interval = check_guidance_interval(guidance_interval)
        if guidance_interval is not None and window_group is not None:
            raise ValueError(f"guidance_interval={tuple(guidance_interval)} is not combined with window_group (the ranks are dealt whole CFG pairs "
                             "or single rows of every step): use one GPU")
        if context_fuse != "flat" and window_group is not None:
            raise ValueError(f"context_fuse={context_fuse!r} is not combined with window_group (the weighted overlap average was never run on more "
                             "than one rank): use context_fuse='flat' or one GPU")
        eta, guidance_rescale = float(eta), float(guidance_rescale)
        dpm = self._check_update_args(eta, guidance_rescale, window_group)
        B = int(context_batch_size)
        if B < 1:
            raise ValueError(f"context_batch_size must be at least 1, got {context_batch_size}")
        if B > 1 and window_group is not None:
            raise ValueError("context_batch_size > 1 is not combined with window_group (window-parallel sampling deals single windows or "
                             "single CFG rows to the ranks): use one of the two")
        return eta, guidance_rescale, dpm, interval, B

    def _cut_units(self, windows, B, video_length, pose_fea, audio, full_masks, face_masks, lip_masks, dev):
        """The pair units of a clip: the window list in its order in groups of B (the last may be smaller), each with its conditioning gathered from
        the full tensors in CFG row major order.  A window at B = 1 is a group of one; only its accumulate index keeps the single window's shape."""
        units = []
        for g0 in range(0, len(windows), B):
            ws = list(range(g0, min(g0 + B, len(windows))))
            if len({len(windows[w]) for w in ws}) != 1:
                raise RuntimeError("context_batch_size > 1: the windows of a group must have the same length")
            idx = torch.tensor([windows[w] for w in ws], device=dev, dtype=torch.int32)           # (n, Fw)
            gl = idx.long()
            rows = lambda t: t.view(2, video_length, -1)[:, gl].reshape(-1, t.shape[-1]).contiguous()     # (2, n, Fw, m) -> (2 n Fw, m)
            units.append(_Unit(ws, None, gl, idx[0] if B == 1 else idx, self._pose_group(pose_fea, list(gl)),
                               audio[:, gl].reshape(2 * len(ws), gl.shape[1], *audio.shape[2:]).contiguous(),
                               [rows(t) for t in full_masks], [rows(t) for t in face_masks], [rows(t) for t in lip_masks]))
        return units

    @staticmethod
    def _check_init_args(init_video, init_latents, strength, regen_mask, paste_back, video_length, window_group, num_images_per_prompt,
                         interpolation_factor, output_type):
        """The refusals of re-voicing's arguments (each names both parties) -> whether an init clip was given."""
        given = [n for n, v in (("init_video", init_video), ("init_latents", init_latents)) if v is not None]
        if len(given) == 2:
            raise ValueError("init_video and init_latents are two forms of the same clip: pass exactly one of them")
        if not given:
            for name, on in ((f"strength={strength}", float(strength) != 1.0), ("regen_mask", regen_mask is not None), ("paste_back", bool(paste_back))):
                if on:
                    raise ValueError(f"{name} changes how an existing clip is re-sampled: it needs init_video or init_latents")
            return False
        init = given[0]
        if window_group is not None:
            raise ValueError(f"{init} is not combined with window_group (re-voicing was never run on more than one rank): use one GPU")
        if num_images_per_prompt > 1:
            raise ValueError(f"{init} is not combined with num_images_per_prompt={num_images_per_prompt}: one init clip gives one clip")
        if interpolation_factor > 1:
            raise ValueError(f"{init} is not combined with interpolation_factor={interpolation_factor}: the interpolated frames have no "
                             "counterpart in the init clip")
        clip = init_video if init_video is not None else init_latents
        n = clip.shape[0] if init_video is not None else (clip.shape[2] if clip.dim() == 5 else -1)
        if n != video_length:
            raise ValueError(f"{init} has {n} frames (shape {tuple(clip.shape)}), video_length={video_length}: the init clip must have the "
                             "sampled clip's length")
        if paste_back and init_video is None:
            raise ValueError("paste_back composites the decoded frames onto the init clip's frames: it needs init_video, not init_latents")
        if paste_back and output_type != "uint8":
            raise ValueError(f'paste_back composites uint8 frames on the device: it needs output_type="uint8", got output_type={output_type!r}')
        return True

    def _init_clip(self, init_video, init_latents, regen_mask, mask_grow, z, width, height, dev):
        """-> (x0 (1, 4, L, h, w) fp32, cell mask (L, h, w) fp32 or None, the init frames at width x height or None), all on the device."""
        from .inputs import resize_frames_device
        frames = None
        if init_video is not None:
            frames = torch.as_tensor(init_video).to(dev)
            if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3:
                raise ValueError(f"init_video: expected uint8 (L, h, w, 3) frames, got {frames.dtype} {tuple(frames.shape)}")
            if tuple(frames.shape[1:3]) != (height, width):
                frames = resize_frames_device(frames, width, height, "lanczos")        # as the reference image
            frames = frames.contiguous()
            if not hasattr(self.vae, "encode_video"):
                raise RuntimeError("init_video needs a VAE with an encoder (AutoencoderKL.encode_video): pass init_latents=(1, 4, L, h, w)")
            x0 = self.vae.encode_video(frames)
        else:
            x0 = init_latents.to(device=dev, dtype=torch.float32).contiguous()
        if tuple(x0.shape) != tuple(z.shape):
            raise ValueError(f"the init clip's latents are {tuple(x0.shape)}, the sampler's {tuple(z.shape)}")
        cells = None
        if regen_mask is not None:
            m = torch.as_tensor(regen_mask).to(dev)
            L, h, w = z.shape[2:]
            if m.dim() != 3 or m.shape[0] != L:
                raise ValueError(f"regen_mask must be (L, H, W) uint8 pixels or (L, h, w) float32 cells with L = {L}, got {tuple(m.shape)}")
            if m.dtype == torch.uint8:
                if tuple(m.shape[1:]) != (height, width):
                    m = resize_frames_device(m[..., None].contiguous(), width, height, "bilinear")[..., 0]
                cells = hip.mask_to_latent(m.contiguous(), mask_grow)
            elif m.dtype == torch.float32 and tuple(m.shape) == (L, h, w):
                cells = m.contiguous()
            else:
                raise ValueError(f"regen_mask must be uint8 (L, H, W) pixels or float32 {(L, h, w)} cells, got {m.dtype} {tuple(m.shape)}")
        return x0, cells, frames

    # --------------------------------------------------------------------------------------------- the hot loop
    def denoise(self, latents, timesteps, encoder_hidden_states, pose_fea, audio_tensor_pre, full_masks, face_masks,
                lip_masks, guidance_scale, motion_scale, context_frames, context_stride, context_overlap,
                context_schedule="uniform", num_inference_steps=None, callback=None, callback_steps=1,
                window_group=None, cfg_split="auto", context_batch_size=1, eta=0.0, guidance_rescale=0.0, generator=None, known=None,
                context_fuse="flat", guidance_interval=None):
        """pipeline_pose2vid_long.py:494-643.  latents (1, C, L, h, w) fp32 on the GPU; returns the final latents.

        A step runs UNITS (`_Unit`): one unit is one call of the operator over 1 to B windows, for the CFG pair or for one CFG row.  The
        scheduler's window list is taken in its order in groups of context_batch_size = B (the last group may be smaller; a window at B = 1 is a
        group of one) and cut ONCE per call into pair units (`_cut_units`), rows in CFG row major order [uncond w0 .. uncond w(n-1), cond w0 ..
        cond w(n-1)]; a single-row unit is a half of its pair's tensors, cut on first use.  Every unit owns its memo for the operator.  `forward`
        is the one call of the operator, `accumulate` the one place a prediction enters pred_sum / counter, and a step is: pick its units, run
        them in list order, update.

        context_batch_size = B > 1 is the SAME sampler as B = 1 with B windows per forward: the predictions are added to pred_sum / counter
        window by window in list order (hip.accumulate_windows), so the fp32 accumulation order of the overlap average is that of B = 1.  Only
        the rounding inside the UNet may differ (dispatch picks tiles by the row count).  The reference's own handling of the argument is
        inconsistent (App. C-7) and is not reproduced.  Not combined with window_group: raises ValueError.

        window_group: a torch.distributed process group (or True for the default group) turns on window-parallel sampling of
        ONE long video.  The units of a DDIM step -- the windows' pairs, or with `cfg_split` both single rows of every
        window -- are dealt round-robin to the ranks; each round ends in ONE all-gather of the units' predictions, sliced
        to the C valid channels (fp32 (rows * Fw, h, w, C): 1.57 MB per CFG row at 24 x 64 x 64 x 4), and every rank then
        accumulates ALL units in the reference's window order and applies the identical overlap-average + CFG + DDIM update --
        so the latents stay bit-identical on every rank, with no other exchange.  cfg_split: "auto" splits the CFG rows when
        that shortens the critical path (6 windows on 4 ranks: 3 rounds of half units instead of 2 rounds of whole ones).

        The update behind the accumulation follows the scheduler's class.  A DDIMScheduler with eta = 0 and guidance_rescale = 0 is
        hip.cfg_ddim_step, as ever.  Anything else is hip.sampler_step: eta > 0 draws one fp32 noise tensor per step from `generator` (after the
        initial latents, in step order); guidance_rescale > 0 scales the guided prediction to the conditional one's standard deviation (the
        moments stay on the device); a DPMSolverMultistepScheduler hands every step's x0 to the next through two buffers allocated here.  All of
        it runs after the gather, so it combines with window_group and context_batch_size -- except eta > 0 with window_group.

        known = (x0, z, mask) keeps a region of an existing clip: after every step's update -- whichever of the above it is -- one
        hip.known_latents launch replaces the cells where the fp32 (L, h, w) mask is 0 by sa x0 + sb z at scheduler.alpha_bar_after(t), in
        place; the callback sees the latents after it.  Behind the last step alpha-bar is 1 and those cells are x0's bits.

        context_schedule="open", context_fuse and guidance_interval are opt-in; with none of them the loop makes the calls it always
        made.  context_fuse = "pyramid" / "ramp" weights the positions of a window in the overlap average (longclip.fuse_weights, rounded once to
        fp32; hip.accumulate_window / accumulate_windows take it as `weights`, add fmaf(w, pred, sum) in list order and counter collects the weights,
        so the update kernels divide by sum w unchanged); one window is always flat.  guidance_interval = (lo, hi) guides the steps with
        lo < (t + 1) / num_train_timesteps <= hi; on every other step ONLY the conditional row runs (cfg_row=1, with a memo of its own), its
        prediction goes to CFG row 1 and the update runs at guidance 1 over the zero row 0 -- v is the conditional average -- without the
        rescale's moments.  Any given guidance_interval, (0, 1) included, and any fuse but "flat" hand the two entries a weight vector (flat: all
        weights 1, the same bits as the `weights=None` of every other call).  Neither is combined with window_group: raises ValueError."""
        from .longclip import fuse_weights, step_is_guided
        eta, guidance_rescale, dpm, interval, B = self._check_loop_args(eta, guidance_rescale, window_group, context_fuse, guidance_interval,
                                                                        context_batch_size)
        if known is not None and window_group is not None:
            raise ValueError("known= (the kept region of an init clip) is not combined with window_group: use one GPU")
        if B > 1 and latents.shape[0] != 1:
            raise ValueError("context_batch_size > 1 batches windows of ONE clip: latents must be (1, C, L, h, w)")
        general = dpm or eta != 0.0 or guidance_rescale != 0.0
        x0_bufs = [torch.empty_like(latents), torch.empty_like(latents)] if dpm else None
        video_length = latents.shape[2]
        dev = latents.device
        sched = get_context_scheduler(context_schedule)
        nsteps = num_inference_steps or len(timesteps)
        # the reference passes step = 0 at every iteration, so the windows never move (:534-543)
        windows = list(sched(0, nsteps, video_length, context_frames, context_stride, context_overlap))
        fuse_w = None
        if context_fuse != "flat" or guidance_interval is not None:     # one fp32 vector per clip; a lone window is averaged with nothing: flat
            if len({len(c) for c in windows}) != 1:
                raise RuntimeError("context_fuse / guidance_interval: the windows of a clip must have the same length")
            fuse_w = torch.tensor(fuse_weights(context_fuse if len(windows) > 1 else "flat", len(windows[0]), context_overlap),
                                  dtype=torch.float64).to(torch.float32).to(dev)
        num_train = getattr(self.scheduler, "num_train_timesteps", 1000)
        # per-window conditioning and the index tensors are step-invariant: cut once per call, single rows on first use
        pairs = self._cut_units(windows, B, video_length, pose_fea, audio_tensor_pre, full_masks, face_masks, lip_masks, dev)
        # the reference's unconditional audio row is zeros_like(audio) (:484-485): checked once here (one device sync per clip), and the
        # operator then skips that row's audio cross-attention, whose result is exactly zero
        hip_op = hasattr(self.denoising_unet, "boc")                # the HIP operator (CPU doubles of the tests take no extras)
        uncond_audio_zero = hip_op and hip.tune_get("zero_audio_skip") and audio_tensor_pre.shape[0] == 2 and \
            not bool(audio_tensor_pre[0].ne(0).any())
        keep_window_state = hip_op and bool(hip.tune_get("window_state"))
        C = latents.shape[1]
        group = world = rank = None
        if window_group is not None:
            group = None if window_group is True else window_group
            world, rank = parallel.dist.get_world_size(group), parallel.dist.get_rank(group)
            nw = len(windows)
            if cfg_split == "auto":
                cfg_split = -(-2 * nw // world) < 2 * -(-nw // world)      # rounds of half units vs rounds of whole units
        split = window_group is not None and bool(cfg_split)

        def forward(u, t):
            """The operator on one unit: (2 n, C, Fw, h, w) in for a pair, (n, C, Fw, h, w) with cfg_row for a single row; ((rows n Fw), h, w, 64)
            channels-last out.  What it tells the operator is true by construction: the pair's second half is .repeat(2 ...) of the first here and
            in _pose_group, the unconditional rows come first, and the memo is the unit's own."""
            lat = self.scheduler.scale_model_input(latents[:, :, u.long].transpose(1, 2).flatten(0, 1), t)      # a gather: window by window
            kw = {}
            if u.row is None:
                lat = lat.repeat(2, 1, 1, 1, 1)
            else:
                lat = lat.contiguous()
                kw["cfg_row"] = u.row
            if keep_window_state:                                # the HIP operator memoises what it derives from the step-invariant inputs
                kw["window_state"] = u.state
            if uncond_audio_zero:
                kw["audio_zero_rows"] = 0 if u.row == 1 else len(u.windows)
            if hip_op and u.row is None:
                kw["cfg_rows_share_input"] = True
            return self.denoising_unet.denoise_window(
                lat, t, encoder_hidden_states=encoder_hidden_states, audio_embedding=u.audio, pose_cond_fea=u.pose,
                full_mask=u.full, face_mask=u.face, body_mask=u.lips, motion_scale=motion_scale, **kw)

        def accumulate(u, pred, pred_sum, counter):
            """One unit's prediction into pred_sum / counter.  The entry follows the call's options, not the unit's size (a lone last group is a group
            of one).  A single row goes to its own CFG row; of a cfg_split pair only row 0 bumps the counter, an unguided step's row 1 bumps it itself."""
            kw = {} if u.row is None else dict(rows=1, row0=u.row)          # only what departs from the pair without weights: the defaults
            if fuse_w is not None:                                          # make the calls they always made
                kw["weights"] = fuse_w
            if B > 1:
                hip.accumulate_windows(pred, pred_sum, counter, u.idx, C, **kw)
            else:
                hip.accumulate_window(pred, pred_sum, counter, u.idx, C, bump_counter=not (split and u.row == 1), **kw)

        def update(i, t, guided, pred_sum, counter):
            """Overlap average + CFG + the scheduler's update -> the next latents.  An unguided step: guidance 1 over the zero row 0 gives
            v = 0 + 1 (c - 0) = c, the conditional average; the rescale is the identity there."""
            g_step = float(guidance_scale) if guided else 1.0
            if not general:
                return hip.cfg_ddim_step(pred_sum, counter, latents, g_step, *self.scheduler.step_coefficients(t))
            noise = None
            if eta > 0.0:                                        # on the generator's device, as the initial latents (prepare_latents)
                gdev = generator.device if isinstance(generator, torch.Generator) else dev
                noise = torch.randn(latents.shape, generator=generator, device=gdev, dtype=torch.float32).to(dev)
            return hip.sampler_step(pred_sum, counter, latents, g_step, *self.scheduler.update_coefficients(t, eta),
                                    rescale=guidance_rescale if guided else 0.0, noise=noise, prev_x0=x0_bufs[(i - 1) % 2] if dpm and i > 0 else None,
                                    x0_out=x0_bufs[i % 2] if dpm else None)

        for i, t in enumerate(timesteps):
            guided = step_is_guided(t, interval, num_train)
            pred_sum = torch.zeros((2,) + tuple(latents.shape[1:]), device=dev, dtype=torch.float32)
            counter = torch.zeros((video_length,), device=dev, dtype=torch.float32)
            # the step's units, in window list order: the pairs; their conditional rows alone on an unguided step; both rows of every pair for cfg_split
            if split:
                units = [p.half(row) for p in pairs for row in (0, 1)]
            else:
                units = pairs if guided else [p.half(1) for p in pairs]
            if window_group is None:
                for u in units:
                    accumulate(u, forward(u, t), pred_sum, counter)
            else:                                                # dealt round-robin to the ranks; every rank accumulates ALL units of a round
                wire_shape = ((1 if split else 2) * len(windows[0]),) + tuple(latents.shape[3:]) + (C,)
                for u0 in range(0, len(units), world):
                    if u0 + rank < len(units):
                        # the operator returns ((rows * Fw), h, w, 64) channels-last with C valid channels: only those travel
                        pred = forward(units[u0 + rank], t)[..., :C].float().contiguous()
                        assert pred.shape == wire_shape, (pred.shape, wire_shape)
                    else:                                   # idle rank in the last round: same shape and dtype on the wire
                        pred = torch.zeros(wire_shape, device=dev, dtype=torch.float32)
                    preds = parallel.allgather_window_predictions(pred, group)
                    for u, p in zip(units[u0:u0 + world], preds):
                        accumulate(u, p, pred_sum, counter)
            latents = update(i, t, guided, pred_sum, counter)
            if known is not None:
                from .scheduler import known_scalars
                hip.known_latents(known[0], known[1], *known_scalars(self.scheduler.alpha_bar_after(t)), x=latents, mask=known[2], out=latents)
            if callback is not None and i % callback_steps == 0:
                callback(i, t, latents)
        return latents

    # --------------------------------------------------------------------------------------------- __call__
    @torch.no_grad()
    def __call__(self, ref_image, pose_images, audio_tensor, pixel_values_full_mask, pixel_values_face_mask,
                 pixel_values_lip_mask, width, height, video_length, num_inference_steps, guidance_scale,
                 num_images_per_prompt=1, eta: float = 0.0, motion_scale: Optional[List[float]] = None,
                 generator=None, output_type: Optional[str] = "tensor", return_dict: bool = True,
                 callback: Optional[Callable] = None, callback_steps: Optional[int] = 1, context_schedule="uniform",
                 context_frames=12, context_stride=1, context_overlap=4, context_batch_size=1, interpolation_factor=1,
                 guidance_rescale: float = 0.0, context_fuse="flat", guidance_interval=None, **kwargs):
        self._check_loop_args(eta, guidance_rescale, kwargs.get("window_group"), context_fuse, guidance_interval, context_batch_size)
        if not guidance_scale > 1.0:
            raise NotImplementedError("classifier-free guidance is mandatory in the reference loop (App. C-7)")
        init_video, init_latents, regen_mask = kwargs.get("init_video"), kwargs.get("init_latents"), kwargs.get("regen_mask")
        strength, paste_back = float(kwargs.get("strength", 1.0)), bool(kwargs.get("paste_back", False))
        revoice = self._check_init_args(init_video, init_latents, strength, regen_mask, paste_back, video_length, kwargs.get("window_group"),
                                        num_images_per_prompt, interpolation_factor, output_type)
        unet = self.denoising_unet
        dev = unet.device
        if revoice:                                              # the last int(N strength) steps of the same schedule
            self.scheduler.set_timesteps(num_inference_steps, device=None, strength=strength)
        else:
            self.scheduler.set_timesteps(num_inference_steps, device=None)
        timesteps = self.scheduler.timesteps

        # ---- prologue (once per clip) -------------------------------------------------------------------
        ref_vae_in = ref_clip_in = None
        if torch.is_tensor(ref_image):          # a uint8 (h, w, 3) image: both resizes and both float stages on the device
            from .inputs import ref_image_tensors_device
            ref_vae_in, ref_clip_in = ref_image_tensors_device(ref_image.to(dev), width, height)
        clip_embeds = kwargs.get("clip_image_embeds")
        if clip_embeds is None:
            if self.image_encoder is None:
                raise RuntimeError("no image_encoder: pass clip_image_embeds=(1, 768)")
            if ref_clip_in is not None:
                clip_image = ref_clip_in
            else:
                from transformers import CLIPImageProcessor
                clip_image = CLIPImageProcessor().preprocess(ref_image.resize((224, 224)), return_tensors="pt").pixel_values
            clip_embeds = self.image_encoder(clip_image.to(dev, dtype=self.image_encoder.dtype)).image_embeds
        ehs = clip_embeds.to(dev).float().reshape(1, 1, -1)
        encoder_hidden_states = torch.cat([torch.zeros_like(ehs), ehs], dim=0)          # :388-394

        banks = kwargs.get("reference_banks")
        if banks is None:
            if self.reference_unet is None:
                raise RuntimeError("no reference_unet: pass reference_banks={prefix: (2, N, C)}")
            ref_latents = kwargs.get("ref_image_latents")
            if ref_latents is None:
                if not hasattr(self.vae, "encode_mean"):
                    raise RuntimeError("the VAE encoder is not part of this build: pass ref_image_latents=(1,4,h,w) "
                                       "(= vae.encode(ref).latent_dist.mean * 0.18215)")
                ref_t = ref_vae_in if ref_vae_in is not None else _pil_to_tensor(ref_image, width, height, True)[None].to(dev)
                ref_latents = self.vae.encode_mean(ref_t) * 0.18215                      # :427-434
            banks = self.reference_unet.write_banks(ref_latents.to(dev).float().repeat(2, 1, 1, 1), 0,
                                                    encoder_hidden_states)               # :510-520
            if unet.bank_fp16_roundtrip:                                                  # update(writer, dtype=fp16): :304,340
                banks = {k: v.to(torch.float16) for k, v in banks.items()}
        unet.set_banks(banks)

        latents = self.prepare_latents(num_images_per_prompt, unet.in_channels, width, height, video_length,
                                       torch.float32, dev, generator, latents=kwargs.get("latents"))
        known = cells = init_frames = None
        if revoice:
            # the noise is the tensor just drawn (init_noise_sigma is 1 on this schedule): no further generator draw.  The start is the init clip
            # noised to timesteps[0]'s alpha-bar; at strength 1 that alpha-bar is exactly 0 (zero terminal SNR) and the start is z's bits
            from .scheduler import known_scalars
            x0, cells, init_frames = self._init_clip(init_video, init_latents, regen_mask, kwargs.get("mask_grow", 1), latents, width, height, dev)
            z = latents
            latents = hip.known_latents(x0, z, *known_scalars(self.scheduler._alpha_bar(int(timesteps[0]))))
            known = (x0, z, cells) if cells is not None else None

        pose_fea = kwargs.get("pose_features")
        if pose_fea is None:
            if torch.is_tensor(pose_images):
                pose_t = pose_images.to(dev).float()
            else:
                pose_t = torch.stack([_pil_to_tensor(p, width, height, False) for p in pose_images], dim=1)[None].to(dev)
            pose_fea = self.pose_guider(pose_t)                                           # :437-448
        pose_fea = pose_fea.to(dev).float()

        dup = lambda ms: [torch.cat([m.to(dev).float()] * 2) for m in ms]                 # :451-482
        full_masks, face_masks, lip_masks = dup(pixel_values_full_mask), dup(pixel_values_face_mask), dup(pixel_values_lip_mask)
        audio = audio_tensor.to(dev).float()
        audio_pre = torch.cat([torch.zeros_like(audio), audio], dim=0)                    # :484-486

        # ---- denoising loop ---------------------------------------------------------------------------------
        latents = self.denoise(latents, timesteps, encoder_hidden_states, pose_fea, audio_pre, full_masks, face_masks,
                               lip_masks, guidance_scale, motion_scale, context_frames, context_stride, context_overlap,
                               context_schedule, num_inference_steps, callback, callback_steps,
                               window_group=kwargs.get("window_group"), cfg_split=kwargs.get("cfg_split", "auto"),
                               context_batch_size=context_batch_size, eta=eta, guidance_rescale=guidance_rescale,
                               generator=generator if isinstance(generator, torch.Generator) else None, known=known,
                               context_fuse=context_fuse, guidance_interval=guidance_interval)
        unet.clear_banks()                                                                # :645-646

        if interpolation_factor > 0:
            latents = self.interpolate_latents(latents, interpolation_factor, dev)
        if not kwargs.get("decode", True):
            return Pose2VideoPipelineOutput(videos=latents) if return_dict else latents
        if output_type == "jpeg":
            images = self.decode_latents_jpeg(latents, kwargs.get("window_group"), kwargs.get("jpeg_quality", 90),
                                              kwargs.get("jpeg_subsampling", "4:2:0"))
            return Pose2VideoPipelineOutput(videos=images) if return_dict else images
        if paste_back:
            # the decoded frames over the init clip's, on the device: alpha is the feathered cell mask (255 everywhere without a mask, where the
            # composite is the decoded frames themselves and is not launched)
            if self.vae is None:
                raise RuntimeError("decode_latents needs a VAE (pass decode=False to get latents)")
            frames = self.vae.decode_video_uint8(latents)                                 # (1, L, H, W, 3)
            if cells is not None:
                alpha = hip.feather_alpha(cells, kwargs.get("feather", 8))
                frames = hip.composite_u8(frames[0].contiguous(), init_frames, alpha)[None]
            images = frames.cpu().numpy()
        else:
            images = self.decode_latents(latents, kwargs.get("window_group"), uint8=output_type == "uint8")
        if output_type in ("tensor", "uint8"):
            images = torch.from_numpy(images)
        if not return_dict:
            return images
        return Pose2VideoPipelineOutput(videos=images)
