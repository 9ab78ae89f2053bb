#!/usr/bin/env python3
"""PNG decoder timings on one MI355X, one JSON line per input; every input is 80 frames of 512 x 512:

  * pil_noise     a directory of PIL-written .png frames of noise-like RGB pixels: nearly all-literal deflate streams
  * pil_masks     a directory of PIL-written .png frames of lines and discs on black: mostly long matches
  * own_apng      the project's own .apng (video_out.encode_png_frames / write_apng) of pose-like frames: distance-1 matches, 8 blocks a frame

Per input: device time of the three launches by HIP events (inflate, unfilter, expand) on operands that are already on the device; and end to
end on the same box, alternating, host clock around work that ends in a synchronise: file -> (1, 3, L, H, W) fp32 pose tensor on the device
through the decoder (read_frames_device -> pose_tensor_device) against the host route (read_frames -> pose_tensor -> .to(device)).  Both routes
give the same tensor; the line says whether they did.

    python tools/bench_pngdec.py [--frames 80] [--reps 20] [--pairs 7] [--out FILE]     (default: rewrites profiles/pngdec/bench_pngdec.jsonl)"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def noise_clip(n, H, W):
    """Smooth colour fields under strong noise: no filter type leaves much to match."""
    rng = np.random.default_rng(20261019)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    out = np.empty((n, H, W, 3), np.uint8)
    for k in range(n):
        f = np.stack([96 + 70 * np.sin(0.013 * (c + 1) * xx + 0.1 * k) * np.cos(0.011 * yy + c) for c in range(3)], axis=-1)
        out[k] = np.clip(f + rng.normal(0, 40, f.shape), 0, 255).astype(np.uint8)
    return out


def mask_clip(n, H, W):
    """Lines and discs on black, as pose frames and binary masks have them."""
    rng = np.random.default_rng(7)
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.zeros((n, H, W, 3), np.uint8)
    for k in range(n):
        for s in range(4):
            cx, cy, r = rng.uniform(0, W), rng.uniform(0, H), rng.uniform(10, 60)
            out[k][(xx - cx) ** 2 + (yy - cy) ** 2 < r * r] = rng.integers(64, 256, 3)
        for s in range(8):
            x0, y0, dx = rng.uniform(0, W), rng.uniform(0, H), rng.uniform(-1, 1)
            out[k][(np.abs((xx - x0) - dx * (yy - y0)) < 2) & (np.abs(yy - y0) < 90)] = rng.integers(64, 256, 3)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--frames", type=int, default=80)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--pairs", type=int, default=7)
    p.add_argument("--out", type=str, default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "pngdec",
                                                           "bench_pngdec.jsonl"))
    a = p.parse_args()
    from PIL import Image
    from mmgt_amd import hip, inputs, video_in, video_out
    dev = torch.device("cuda:0")
    n, H, W = a.frames, 512, 512
    tmp = tempfile.mkdtemp(prefix="bench_pngdec_")
    paths = {}
    for name, frames in (("pil_noise", noise_clip(n, H, W)), ("pil_masks", mask_clip(n, H, W))):
        paths[name] = os.path.join(tmp, name)
        os.makedirs(paths[name])
        for k in range(n):
            Image.fromarray(frames[k]).save(os.path.join(paths[name], f"{k:04d}.png"))
    paths["own_apng"] = os.path.join(tmp, "clip.apng")
    video_out.write_apng(paths["own_apng"], video_out.encode_png_frames(torch.from_numpy(mask_clip(n, H, W)).to(dev)), W, H, 25)
    lines = []
    for name, path in paths.items():
        files = [open(path, "rb").read()] if os.path.isfile(path) else [open(os.path.join(path, f), "rb").read() for f in sorted(os.listdir(path))]
        headers, (_, _, ct, depth), data, offsets, adlers, _, _ = video_in.png_batch_operands(files)
        stride = headers[0].stride
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
        d_data, d_off = up(data.copy()), up(offsets)
        filt, status = hip.png_inflate(d_data, d_off, H * stride)
        sums, st1 = hip.png_unfilter(filt, H, W, ct, depth)
        out, st2 = hip.png_expand(filt, H, W, ct, depth)
        assert not bool(status.any()) and not bool(st1.any()) and np.array_equal(video_in.adler32_of_row_sums(sums.cpu().numpy(), stride), adlers)
        lib, st = hip.lib(), torch.cuda.current_stream().cuda_stream
        t_inf = timed(lambda: lib.mmgt_png_inflate(d_data.data_ptr(), d_data.numel(), d_off.data_ptr(), filt.data_ptr(), status.data_ptr(), n,
                                                   H * stride, st), a.reps)
        t_unf = timed(lambda: lib.mmgt_png_unfilter(filt.data_ptr(), sums.data_ptr(), st1.data_ptr(), n, H, W, ct, depth, st), a.reps)
        t_exp = timed(lambda: lib.mmgt_png_expand(filt.data_ptr(), None, None, out.data_ptr(), st2.data_ptr(), n, H, W, ct, depth, st), a.reps)

        def device_route():
            return inputs.pose_tensor_device(video_in.read_frames_device(path, n, dev), W, H)

        def host_route():
            return inputs.pose_tensor(inputs.read_frames(path, n), W, H).to(dev)
        same = bool(torch.equal(device_route(), host_route()))                                  # also warms both
        dev_s, host_s = [], []
        for _ in range(a.pairs):
            for f, acc in ((device_route, dev_s), (host_route, host_s)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()
                torch.cuda.synchronize()
                acc.append(time.perf_counter() - t0)
        med = lambda v: sorted(v)[len(v) // 2]
        rec = {"input": name, "frames": n, "size": [H, W], "colour_type": ct, "bit_depth": depth, "bytes_in": int(offsets[-1]),
               "bytes_inflated": int(n * H * stride), "box": torch.cuda.get_device_name(0), "device_equals_host_route": same,
               "inflate_ms": round(t_inf, 3), "unfilter_ms": round(t_unf, 3), "expand_ms": round(t_exp, 3),
               "kernels_ms_per_frame": round((t_inf + t_unf + t_exp) / n, 4),
               "device_route_ms": [round(1e3 * t, 2) for t in dev_s], "host_route_ms": [round(1e3 * t, 2) for t in host_s],
               "device_route_ms_per_frame_median": round(1e3 * med(dev_s) / n, 3), "host_route_ms_per_frame_median": round(1e3 * med(host_s) / n, 3)}
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
    shutil.rmtree(tmp, ignore_errors=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
