#!/usr/bin/env python3
"""What several context windows per forward (`context_batch_size` = B, DESIGN.md "Several windows per forward") cost or buy on one MI355X.

512 x 512, bf16, guidance 3.5, random-init weights of the reference architecture, `Pose2VideoPipeline.denoise` alone between HIP events,
ms per DDIM step, in two geometries:

  * 80 frames, windows of 12, overlap 4 (the shipped settings: 10 windows per step);
  * 96 frames, windows of 24, overlap 4 (5 windows per step).

For every B in {2, 4, all windows} the run alternates B = 1 / B = k pairs in ONE process on the same box (`--pairs`, at least five), after a
warm-up of both; the yardstick of every B is the B = 1 of its own pairs.  One JSON line per (geometry, B) with every sample, the medians,
the spread (min .. max) and the median of the per-pair ratios; the lines of the run are written to profiles/ctxbatch/bench_ctxbatch.jsonl (--out).

    python tools/bench_ctxbatch.py [--pairs 5] [--steps 2] [--batches 2,4,all] [--geometries 80:12:4,96:24:4] [--out FILE]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--pairs", type=int, default=5)
    p.add_argument("--steps", type=int, default=2, help="DDIM steps per timed denoise call")
    p.add_argument("--batches", type=str, default="2,4,all")
    p.add_argument("--geometries", type=str, default="80:12:4,96:24:4", help="frames:context:overlap, comma separated")
    p.add_argument("--out", type=str, default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ctxbatch",
                                                          "bench_ctxbatch.jsonl"), help="the lines of this run (the file is rewritten)")
    a = p.parse_args()
    from mmgt_amd.context import uniform
    from mmgt_amd.pipeline import Pose2VideoPipeline
    from mmgt_amd.scheduler import DDIMScheduler
    from mmgt_amd.synthetic import bank_spatial, hash_uniform, synth_masks, synth_state_dict
    from mmgt_amd.unet3d import UNet3DConditionModel
    from mmgt_amd.unet3d_spec import unet3d_spec
    dev = torch.device("cuda:0")
    unet = UNet3DConditionModel(device=dev, dtype=torch.bfloat16)
    unet.load_state_dict(synth_state_dict(unet3d_spec(), device=dev))
    unet.enable_gradient_checkpointing()
    sched = DDIMScheduler()
    sched.set_timesteps(25)
    pipe = Pose2VideoPipeline(vae=None, image_encoder=None, reference_unet=None, denoising_unet=unet, pose_guider=None, scheduler=sched)
    lines = []
    for geo in a.geometries.split(","):
        frames, ctx, ov = (int(x) for x in geo.split(":"))
        tag, latent = f"bench.ctxbatch.{frames}", 64
        lips, face = synth_masks(tag + ".lips", frames, latent), synth_masks(tag + ".face", frames, latent)
        dup = lambda ms: [torch.cat([m] * 2).to(dev) for m in ms]
        full, face, lips = dup([1 + l for l in lips]), dup(face), dup(lips)
        latents = hash_uniform(tag + ".latents", (1, 4, frames, latent, latent), 1.7).to(dev)
        audio = hash_uniform(tag + ".audio", (1, frames, 32, 768), 1.7).to(dev)
        audio_pre = torch.cat([torch.zeros_like(audio), audio])
        pose = hash_uniform(tag + ".pose", (1, 320, frames, latent, latent), 0.5).to(dev)
        ehs = torch.cat([torch.zeros(1, 1, 768, device=dev), hash_uniform(tag + ".clip", (1, 1, 768), 1.0).to(dev)])
        unet.set_banks({k: hash_uniform(tag + ".bank." + k, (2, n, c), 1.0).to(dev)
                        for k, (n, c) in bank_spatial((320, 640, 1280, 1280), latent).items()})
        nwin = len(list(uniform(0, 25, frames, ctx, 1, ov)))
        ts = [sched.timesteps[3 + i] for i in range(a.steps)]

        def step_ms(B):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            out = pipe.denoise(latents, ts, ehs, pose, audio_pre, full, face, lips, 3.5, [1.0, 1.0, 2.0], context_frames=ctx, context_stride=1,
                               context_overlap=ov, num_inference_steps=25, context_batch_size=B)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / a.steps, out

        base_out = step_ms(1)[1]                                   # warm-up of B = 1 (allocator, dispatch tables)
        for b in a.batches.split(","):
            B = nwin if b == "all" else int(b)
            if B > nwin:
                continue
            rec = {"frames": frames, "context_frames": ctx, "context_overlap": ov, "windows_per_step": nwin, "context_batch_size": B,
                   "forwards_per_step": -(-nwin // B), "size": [512, 512], "dtype": "bf16", "steps_per_sample": a.steps,
                   "box": torch.cuda.get_device_name(0)}
            try:
                out = step_ms(B)[1]                                # warm-up of B = k
            except RuntimeError as e:                              # a group the operator refuses (2 GiB operands): recorded, not timed
                if "2 GiB" not in str(e):
                    raise
                rec["refused"] = str(e)[:300]
                print(json.dumps(rec), flush=True)
                lines.append(json.dumps(rec))
                continue
            assert torch.isfinite(out).all()
            d = (out - base_out).abs()
            rec["max_abs_delta_vs_b1"], rec["mean_abs_delta_vs_b1"] = d.max().item(), d.mean().item()
            one, many = [], []
            for _ in range(max(a.pairs, 5)):
                one.append(step_ms(1)[0])
                many.append(step_ms(B)[0])
            med = lambda v: sorted(v)[len(v) // 2]
            rec.update(b1_ms_per_step=[round(x, 2) for x in one], bk_ms_per_step=[round(x, 2) for x in many],
                       b1_median=round(med(one), 2), bk_median=round(med(many), 2), b1_spread=[round(min(one), 2), round(max(one), 2)],
                       bk_spread=[round(min(many), 2), round(max(many), 2)],
                       ratio_bk_over_b1_median=round(med([m / o for m, o in zip(many, one)]), 4),
                       ms_per_frame_forward_b1=round(med(one) / (nwin * ctx), 3), ms_per_frame_forward_bk=round(med(many) / (nwin * ctx), 3))
            print(json.dumps(rec), flush=True)
            lines.append(json.dumps(rec))
            del out
            torch.cuda.empty_cache()
        del base_out
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
