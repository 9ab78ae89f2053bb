#!/usr/bin/env python3
"""What the sampler's update costs on one MI355X: the launches of csrc/sampler.hip beside `cfg_ddim_step`, at the latents of an 80-frame 512 x 512 clip,
(1, 4, 80, 64, 64) fp32 = 5.2 MB per tensor.

Per variant: `--reps` windows of `--iters` back-to-back calls between HIP events after `--warmup` calls, us per call (median and spread of the windows),
the bytes the call must move (computed from the shapes: every operand read once, every result written once) and the rate that makes.  One JSON line per
variant; the lines of the run are written to profiles/sampler/bench_sampler.jsonl (--out; the file is rewritten).

    python tools/bench_sampler.py [--iters 200] [--reps 7] [--warmup 20] [--out FILE]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=200)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--shape", type=str, default="4,80,64,64", help="C,F,H,W of the latents")
    p.add_argument("--out", type=str, default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "sampler",
                                                          "bench_sampler.jsonl"), help="the lines of this run (the file is rewritten)")
    a = p.parse_args()
    from mmgt_amd import hip
    from mmgt_amd.scheduler import DDIMScheduler, DPMSolverMultistepScheduler
    from mmgt_amd.synthetic import hash_uniform
    dev = torch.device("cuda:0")
    C, F, H, W = (int(v) for v in a.shape.split(","))
    n = C * F * H * W
    cnt = (1.0 + (torch.arange(F, device=dev) % 2).float()).contiguous()
    ps = (hash_uniform("bench.sampler.ps", (2, C, F, H, W), 1.0).to(dev) * cnt[None, None, :, None, None]).contiguous()
    lat, xp, z = (hash_uniform("bench.sampler." + k, (1, C, F, H, W), 1.5).to(dev) for k in ("lat", "xp", "z"))
    out, x0 = torch.empty_like(lat), torch.empty_like(lat)
    mom = torch.empty(4, device=dev, dtype=torch.float64)
    ddim, dpm = DDIMScheduler(), DPMSolverMultistepScheduler()
    ddim.set_timesteps(25)
    dpm.set_timesteps(25)
    t = int(ddim.timesteps[12])
    old, eta, dp2 = ddim.step_coefficients(t), ddim.update_coefficients(t, 0.7), dpm.update_coefficients(t)
    assert dp2[4] != 0.0 and eta[6] != 0.0
    variants = [       # (name, tensors of n floats moved, call)
        ("cfg_ddim_step", 4, lambda: hip.cfg_ddim_step(ps, cnt, lat, 3.5, *old, out=out)),
        ("sampler_step ddim eta=0.7", 5, lambda: hip.sampler_step(ps, cnt, lat, 3.5, *eta, noise=z, out=out)),
        ("sampler_step dpmpp2m second order", 6, lambda: hip.sampler_step(ps, cnt, lat, 3.5, *dp2, prev_x0=xp, x0_out=x0, out=out)),
        ("cfg_moments", 2, lambda: hip.cfg_moments(ps, cnt, 3.5, out=mom)),
        ("cfg_moments + sampler_step dpmpp2m rescale=0.7", 8,
         lambda: hip.sampler_step(ps, cnt, lat, 3.5, *dp2, rescale=0.7, moments=hip.cfg_moments(ps, cnt, 3.5, out=mom), prev_x0=xp, x0_out=x0, out=out)),
    ]
    lines = []
    for name, tensors, call in variants:
        for _ in range(a.warmup):
            call()
        samples = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.iters):
                call()
            e1.record()
            torch.cuda.synchronize()
            samples.append(e0.elapsed_time(e1) * 1e3 / a.iters)
        assert torch.isfinite(out).all()
        med = sorted(samples)[len(samples) // 2]
        rec = {"variant": name, "shape": [1, C, F, H, W], "us_per_call_median": round(med, 2), "us_per_call_spread": [round(min(samples), 2), round(max(samples), 2)],
               "bytes_moved": tensors * n * 4, "gb_per_s_at_median": round(tensors * n * 4 / med / 1e3, 1), "iters": a.iters, "reps": a.reps,
               "includes": "host launch path (ctypes binding, allocator) of back-to-back calls", "box": torch.cuda.get_device_name(0)}
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
