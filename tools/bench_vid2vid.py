#!/usr/bin/env python3
"""What re-voicing an existing clip costs on one MI355X: the four launches of csrc/vid2vid.hip at the sizes of an 80-frame 512 x 512 clip --
latents (1, 4, 80, 64, 64) fp32, frames 80 x 512 x 512 uint8 -- the per-step blend beside `cfg_ddim_step`, and `AutoencoderKL.encode_video` per frame.

Per variant: `--reps` windows of `--iters` back-to-back calls between HIP events after `--warmup` calls, us per call (median and spread of the windows),
the bytes the call must move (from the shapes: every operand read once, every result written once) and the rate that makes.  The encoder (random
weights, bf16 and fp32) is timed in windows of one call over 8 frames, reported as ms per frame.  One JSON line per variant; the lines of the run are
written to profiles/vid2vid/bench_vid2vid.jsonl (--out; the file is rewritten).

    python tools/bench_vid2vid.py [--iters 100] [--reps 7] [--warmup 10] [--no-encoder] [--out FILE]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(call, iters, reps, warmup):
    for _ in range(warmup):
        call()
    samples = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(iters):
            call()
        e1.record()
        torch.cuda.synchronize()
        samples.append(e0.elapsed_time(e1) * 1e3 / iters)
    return sorted(samples)[len(samples) // 2], min(samples), max(samples)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=100)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--frames", type=int, default=80)
    p.add_argument("--size", type=int, default=512, help="frame height and width in pixels")
    p.add_argument("--no-encoder", action="store_true")
    p.add_argument("--out", type=str, default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "vid2vid",
                                                          "bench_vid2vid.jsonl"), help="the lines of this run (the file is rewritten)")
    a = p.parse_args()
    from mmgt_amd import hip
    from mmgt_amd.scheduler import DDIMScheduler
    from mmgt_amd.synthetic import hash_uniform
    dev = torch.device("cuda:0")
    L, S = a.frames, a.size
    h = S // 8
    n, npix = 4 * L * h * h, L * S * S
    x0, z, x = (hash_uniform("bench.v2v." + k, (1, 4, L, h, h), 1.5).to(dev) for k in ("x0", "z", "x"))
    out = torch.empty_like(x0)
    yy, xx = torch.meshgrid(torch.arange(S, device=dev), torch.arange(S, device=dev), indexing="ij")
    px = ((((yy - 0.6 * S) ** 2 + (xx - 0.5 * S) ** 2) < (0.12 * S) ** 2).to(torch.uint8) * 255)[None].repeat(L, 1, 1).contiguous()   # a mouth-sized disc
    cells = hip.mask_to_latent(px, 1)
    gen, orig = (torch.randint(0, 256, (L, S, S, 3), dtype=torch.uint8, device=dev) for _ in range(2))
    alpha = hip.feather_alpha(cells, 8)
    comp = torch.empty_like(gen)
    cnt = (1.0 + (torch.arange(L, device=dev) % 2).float()).contiguous()
    ps = (hash_uniform("bench.v2v.ps", (2, 4, L, h, h), 1.0).to(dev) * cnt[None, None, :, None, None]).contiguous()
    ddim = DDIMScheduler()
    ddim.set_timesteps(25)
    co = ddim.step_coefficients(int(ddim.timesteps[12]))
    variants = [       # (name, bytes moved, call)
        ("known_latents (the start)", 3 * n * 4, lambda: hip.known_latents(x0, z, 0.6, 0.8, out=out)),
        ("known_latents with mask (the per-step blend, in place)", 4 * n * 4 + L * h * h * 4, lambda: hip.known_latents(x0, z, 0.6, 0.8, x=x, mask=cells, out=x)),
        ("cfg_ddim_step (the step the blend follows)", 4 * n * 4, lambda: hip.cfg_ddim_step(ps, cnt, x0, 3.5, *co, out=out)),
        ("mask_to_latent grow=1", npix + L * h * h * 4, lambda: hip.mask_to_latent(px, 1)),
        ("mask_to_latent grow=8", npix + L * h * h * 4, lambda: hip.mask_to_latent(px, 8)),
        ("feather_alpha r=8", npix + L * h * h * 4, lambda: hip.feather_alpha(cells, 8)),
        ("feather_alpha r=32", npix + L * h * h * 4, lambda: hip.feather_alpha(cells, 32)),
        ("composite_u8", 10 * npix, lambda: hip.composite_u8(gen, orig, alpha, out=comp)),
    ]
    lines = []
    for name, nbytes, call in variants:
        med, lo, hi = timed(call, a.iters, a.reps, a.warmup)
        rec = {"variant": name, "latents": [1, 4, L, h, h], "frames": [L, S, S], "us_per_call_median": round(med, 2), "us_per_call_spread": [round(lo, 2), round(hi, 2)],
               "bytes_moved": nbytes, "gb_per_s_at_median": round(nbytes / med / 1e3, 1), "iters": a.iters, "reps": a.reps,
               "includes": "host launch path (ctypes binding, allocator) of back-to-back calls", "box": torch.cuda.get_device_name(0)}
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
    if not a.no_encoder:
        from mmgt_amd.synthetic import synth_state_dict
        from mmgt_amd.vae import AutoencoderKL, vae_decoder_spec, vae_encoder_spec
        frames = gen[:8].contiguous()
        spec = vae_decoder_spec()
        spec.update(vae_encoder_spec())
        for dtype in (torch.bfloat16, torch.float32):
            vae = AutoencoderKL(device=dev, dtype=dtype)
            vae.load_state_dict(synth_state_dict(spec, prefix="vae.", device=dev))
            med, lo, hi = timed(lambda: vae.encode_video(frames), 1, a.reps, 2)
            rec = {"variant": f"encode_video {str(dtype).split('.')[-1]}", "frames": [8, S, S], "ms_per_frame_median": round(med / 8e3, 3),
                   "ms_per_frame_spread": [round(lo / 8e3, 3), round(hi / 8e3, 3)], "reps": a.reps, "box": torch.cuda.get_device_name(0)}
            print(json.dumps(rec), flush=True)
            lines.append(json.dumps(rec))
            del vae
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
