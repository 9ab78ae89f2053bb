#!/usr/bin/env python3
"""What the long-clip options of the sampler (open-ended windows, weighted window blending, guidance interval) cost or buy on one MI355X.

bf16, guidance 3.5, random-init weights of the reference architecture, `Pose2VideoPipeline.denoise` alone between HIP events, every comparison in
alternating pairs in ONE process on the same box (`--pairs`, at least five) after a warm-up of both sides.  Three kinds of line:

  * "accumulate": us per launch of mmgt_accumulate_windows with a weight vector beside the same entry without one at B = 4, Fw = 12, 64 x 64
    latents, C = 4, Cpad = 64 (bf16 predictions, open windows of a 36-frame clip), `--launches` launches per sample;
  * "forward": ms per step of a step that runs the CFG pair beside a step that runs the conditional row alone -- 512 x 512 x 24 in one window, and
    512 x 512 x 80 at windows of 12 / 4 with context_batch_size 1 and 4.  Both sides hand the entries a weight vector (guidance_interval = (0, 1)
    against an interval that holds no step), so only the forward and the skipped row differ;
  * "clip": ms per 80-frame clip at 25 steps, uniform / flat / every step guided (the defaults) beside open / pyramid / guidance_interval
    (0.25, 0.75).

The first block of the operator is already shared between the two CFG rows and the zero-audio row's cross-attention is already skipped, so the
conditional row alone is expected to save less than half of a pair.  One JSON line per comparison with every sample, the medians, the spread and
the median of the per-pair ratios; the lines of the run are written to profiles/longclip/bench_longclip.jsonl (--out; the file is rewritten).

    python tools/bench_longclip.py [--pairs 5] [--steps 2] [--clip_steps 25] [--launches 200] [--skip accumulate,forward,clip] [--out FILE]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NO_STEP = (0.0, 1e-4)            # u = (t + 1) / 1000 >= 1e-3 at every timestep: no step is guided


def med(v):
    return sorted(v)[len(v) // 2]


def paired(rec, a_name, b_name, fn_a, fn_b, pairs, digits=2):
    """alternate fn_a / fn_b `pairs` times (both warmed by the caller) and add samples, medians, spreads and the median per-pair ratio b / a to rec"""
    xs, ys = [], []
    for _ in range(max(pairs, 5)):
        xs.append(fn_a())
        ys.append(fn_b())
    r = lambda v: round(v, digits)
    rec.update({a_name: [r(x) for x in xs], b_name: [r(y) for y in ys], a_name + "_median": r(med(xs)), b_name + "_median": r(med(ys)),
                a_name + "_spread": [r(min(xs)), r(max(xs))], b_name + "_spread": [r(min(ys)), r(max(ys))],
                f"ratio_{b_name}_over_{a_name}_median": round(med([y / x for x, y in zip(xs, ys)]), 4)})
    return rec


def bench_accumulate(a, dev):
    from mmgt_amd import hip
    from mmgt_amd.longclip import fuse_weights, open_ended
    from mmgt_amd.synthetic import hash_uniform
    B, Fw, F, C, cpad, hw = 4, 12, 36, 4, 64, 64
    wins = list(open_ended(0, 25, F, Fw, 1, 4))
    assert len(wins) == B
    idx = torch.tensor(wins, device=dev, dtype=torch.int32)
    pred = hash_uniform("bench.longclip.pred", (2 * B * Fw, hw, hw, cpad), 1.0).to(dev).to(torch.bfloat16)
    w = torch.tensor(fuse_weights("pyramid", Fw), dtype=torch.float32, device=dev)
    ps, cnt = torch.zeros((2, C, F, hw, hw), device=dev), torch.zeros(F, device=dev)

    def us(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.launches):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.launches
    flat = lambda: hip.accumulate_windows(pred, ps, cnt, idx, C)
    weighted = lambda: hip.accumulate_windows(pred, ps, cnt, idx, C, weights=w)
    us(flat), us(weighted)
    rec = {"kind": "accumulate", "B": B, "Fw": Fw, "F": F, "C": C, "Cpad": cpad, "latent": [hw, hw], "pred": "bf16", "launches_per_sample": a.launches,
           "bytes_read_pred": pred.numel() * 2, "box": torch.cuda.get_device_name(0)}
    return [paired(rec, "flat_us", "weighted_us", lambda: us(flat), lambda: us(weighted), a.pairs, 3)]


def bench_denoise(a, dev, kinds):
    from mmgt_amd.longclip import get_context_scheduler
    from mmgt_amd.pipeline import Pose2VideoPipeline
    from mmgt_amd.scheduler import DDIMScheduler
    from mmgt_amd.synthetic import bank_spatial, hash_uniform, synth_masks, synth_state_dict
    from mmgt_amd.unet3d import UNet3DConditionModel
    from mmgt_amd.unet3d_spec import unet3d_spec
    unet = UNet3DConditionModel(device=dev, dtype=torch.bfloat16)
    unet.load_state_dict(synth_state_dict(unet3d_spec(), device=dev))
    unet.enable_gradient_checkpointing()
    sched = DDIMScheduler()
    sched.set_timesteps(a.clip_steps)
    pipe = Pose2VideoPipeline(vae=None, image_encoder=None, reference_unet=None, denoising_unet=unet, pose_guider=None, scheduler=sched)
    lines, latent = [], 64

    def inputs(frames):
        tag = f"bench.longclip.{frames}"
        lips, face = synth_masks(tag + ".lips", frames, latent), synth_masks(tag + ".face", frames, latent)
        dup = lambda ms: [torch.cat([m] * 2).to(dev) for m in ms]
        audio = hash_uniform(tag + ".audio", (1, frames, 32, 768), 1.7).to(dev)
        unet.set_banks({k: hash_uniform(tag + ".bank." + k, (2, n, c), 1.0).to(dev) for k, (n, c) in bank_spatial((320, 640, 1280, 1280), latent).items()})
        return dict(latents=hash_uniform(tag + ".latents", (1, 4, frames, latent, latent), 1.7).to(dev),
                    audio_pre=torch.cat([torch.zeros_like(audio), audio]), pose=hash_uniform(tag + ".pose", (1, 320, frames, latent, latent), 0.5).to(dev),
                    ehs=torch.cat([torch.zeros(1, 1, 768, device=dev), hash_uniform(tag + ".clip", (1, 1, 768), 1.0).to(dev)]),
                    full=dup([1 + l for l in lips]), face=dup(face), lips=dup(lips))

    def run_ms(inp, ts, ctx, ov, **kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        out = pipe.denoise(inp["latents"], ts, inp["ehs"], inp["pose"], inp["audio_pre"], inp["full"], inp["face"], inp["lips"], 3.5, [1.0, 1.0, 2.0],
                           context_frames=ctx, context_stride=1, context_overlap=ov, num_inference_steps=a.clip_steps, **kw)
        e1.record()
        torch.cuda.synchronize()
        assert torch.isfinite(out).all()
        return e0.elapsed_time(e1)

    base = {"size": [512, 512], "dtype": "bf16", "box": torch.cuda.get_device_name(0)}
    if "forward" in kinds:
        ts = [sched.timesteps[3 + i] for i in range(a.steps)]
        for frames, ctx, ov, B in ((24, 24, 4, 1), (80, 12, 4, 1), (80, 12, 4, 4)):
            inp = inputs(frames)
            pair = lambda: run_ms(inp, ts, ctx, ov, context_batch_size=B, guidance_interval=(0, 1)) / a.steps
            cond = lambda: run_ms(inp, ts, ctx, ov, context_batch_size=B, guidance_interval=NO_STEP) / a.steps
            pair(), cond()
            rec = dict(base, kind="forward", frames=frames, context_frames=ctx, context_overlap=ov, context_batch_size=B, steps_per_sample=a.steps,
                       windows_per_step=len(list(get_context_scheduler("uniform")(0, a.clip_steps, frames, ctx, 1, ov))))
            lines.append(paired(rec, "pair_ms_per_step", "cond_only_ms_per_step", pair, cond, a.pairs))
            print(json.dumps(lines[-1]), flush=True)
            del inp
            torch.cuda.empty_cache()
    if "clip" in kinds:
        from mmgt_amd.longclip import check_guidance_interval, step_is_guided
        frames, ctx, ov = 80, 12, 4
        inp, ts = inputs(frames), list(sched.timesteps)
        new = dict(context_schedule="open", context_fuse="pyramid", guidance_interval=(0.25, 0.75))
        old_clip = lambda: run_ms(inp, ts, ctx, ov)
        new_clip = lambda: run_ms(inp, ts, ctx, ov, **new)
        old_clip(), new_clip()
        rec = dict(base, kind="clip", frames=frames, context_frames=ctx, context_overlap=ov, context_batch_size=1, steps=a.clip_steps,
                   windows_per_step=[len(list(get_context_scheduler(n)(0, a.clip_steps, frames, ctx, 1, ov))) for n in ("uniform", "open")],
                   guided_steps=sum(step_is_guided(int(t), check_guidance_interval(new["guidance_interval"])) for t in ts),
                   new={k: list(v) if isinstance(v, tuple) else v for k, v in new.items()})
        lines.append(paired(rec, "default_ms_per_clip", "longclip_ms_per_clip", old_clip, new_clip, a.pairs, 1))
        print(json.dumps(lines[-1]), flush=True)
    return lines


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--pairs", type=int, default=5)
    p.add_argument("--steps", type=int, default=2, help="steps per timed denoise call of the forward lines")
    p.add_argument("--clip_steps", type=int, default=25, help="the schedule's length, and the steps of a clip")
    p.add_argument("--launches", type=int, default=200, help="launches per sample of the accumulate line")
    p.add_argument("--skip", type=str, default="", help="comma separated kinds to leave out: accumulate, forward, clip")
    p.add_argument("--out", type=str, default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "longclip",
                                                          "bench_longclip.jsonl"), help="the lines of this run (the file is rewritten)")
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_longclip needs an MI355X (nothing here is measured on a CPU)")
    dev = torch.device("cuda:0")
    kinds = [k for k in ("accumulate", "forward", "clip") if k not in a.skip.split(",")]
    lines = []
    if "accumulate" in kinds:
        lines += bench_accumulate(a, dev)
        print(json.dumps(lines[-1]), flush=True)
    if "forward" in kinds or "clip" in kinds:
        lines += bench_denoise(a, dev, kinds)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(json.dumps(l) for l in lines) + "\n")


if __name__ == "__main__":
    main()
