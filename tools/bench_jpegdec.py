#!/usr/bin/env python3
"""JPEG decoder timings on one MI355X, one JSON line per input; both inputs are 80 frames of 512 x 512, 4:2:0:

  * avi_32_segments    a Motion-JPEG .avi from video_out.write_avi: one restart interval per MCU row, 32 segments (= lanes) per frame
  * jpg_1_segment      a directory of PIL-written .jpg frames without DRI: one segment per frame, so 80 lanes decode the clip

Per input: device time of the three launches by HIP events (entropy with its zero fill, idct, colour) on operands that are already on the device;
and end to end on the same box, alternating, host clock around work that ends in a synchronise: file -> (1, 3, L, H, W) fp32 pose tensor on the
device through the decoder (read_frames_device -> pose_tensor_device) against the host route (read_frames -> pose_tensor -> .to(device)).
Both routes give the same tensor when PIL is built on libjpeg-turbo; the line says whether they did.

    python tools/bench_jpegdec.py [--frames 80] [--reps 20] [--pairs 7] [--out FILE]     (default: rewrites profiles/jpegdec/bench_jpegdec.jsonl)"""
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


def clip(n, H, W):
    """Seeded frames with the statistics of a rendered pose clip: smooth colour fields, a few hard-edged bright strokes, mild noise."""
    rng = np.random.default_rng(20261018)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    out = np.empty((n, H, W, 3), np.uint8)
    for k in range(n):
        f = np.stack([96 + 70 * np.sin(0.013 * (c + 1) * xx + 0.1 * k) * np.cos(0.011 * yy + c) for c in range(3)], axis=-1)
        for s in range(6):
            cx, cy = rng.uniform(0, W), rng.uniform(0, H)
            f[(np.abs(xx - cx) < 4 + s) & (np.abs(yy - cy) < 60)] = rng.uniform(120, 255, 3)
        out[k] = np.clip(f + rng.normal(0, 3, f.shape), 0, 255).astype(np.uint8)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--frames", type=int, default=80)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--pairs", type=int, default=7)
    p.add_argument("--quality", type=int, default=90)
    p.add_argument("--out", type=str, default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "jpegdec",
                                                           "bench_jpegdec.jsonl"))
    a = p.parse_args()
    from PIL import Image, features
    from mmgt_amd import hip, inputs, video_in, video_out
    dev = torch.device("cuda:0")
    n, H, W = a.frames, 512, 512
    frames = clip(n, H, W)
    tmp = tempfile.mkdtemp(prefix="bench_jpegdec_")
    avi = os.path.join(tmp, "clip.avi")
    video_out.write_avi(avi, video_out.encode_jpeg_frames(torch.from_numpy(frames).to(dev), a.quality, "4:2:0"), W, H, 25)
    jpg_dir = os.path.join(tmp, "frames")
    os.makedirs(jpg_dir)
    for k in range(n):
        Image.fromarray(frames[k]).save(os.path.join(jpg_dir, f"{k:04d}.jpg"), quality=a.quality, subsampling=2)
    lines = []
    for name, path in (("avi_32_segments", avi), ("jpg_1_segment", jpg_dir)):
        jpegs = inputs.mjpeg_avi_frames(path) if path == avi else [open(os.path.join(jpg_dir, f), "rb").read() for f in sorted(os.listdir(jpg_dir))]
        headers, data, offsets, seginfo, tables = video_in.batch_operands(jpegs)
        geo = headers[0].geometry
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
        d_data, d_off, d_seg, d_tab = up(data.copy()), up(offsets), up(seginfo), up(tables)
        coef, status = hip.jpegdec_entropy(d_data, d_off, d_seg, d_tab, n, *geo)
        assert int(status.abs().sum()) == 0
        planes = hip.jpegdec_idct(coef, d_tab, *geo)
        out = hip.jpegdec_color(planes, *geo)
        lib, st = hip.lib(), torch.cuda.current_stream().cuda_stream
        t_ent = timed(lambda: lib.mmgt_jpegdec_entropy(d_data.data_ptr(), d_data.numel(), d_off.data_ptr(), d_seg.data_ptr(), d_tab.data_ptr(),
                                                       coef.data_ptr(), status.data_ptr(), n, len(seginfo), *geo, st), a.reps)
        t_idct = timed(lambda: lib.mmgt_jpegdec_idct(coef.data_ptr(), d_tab.data_ptr(), planes.data_ptr(), n, *geo, st), a.reps)
        t_col = timed(lambda: lib.mmgt_jpegdec_color(planes.data_ptr(), out.data_ptr(), n, *geo, st), a.reps)

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
        rec = {"input": name, "frames": n, "size": [H, W], "subsampling": "4:2:0", "quality": a.quality, "segments_per_frame": len(seginfo) // n,
               "bytes_in": int(data.size), "box": torch.cuda.get_device_name(0), "pil_libjpeg_turbo": bool(features.check_feature("libjpeg_turbo")),
               "device_equals_host_route": same,
               "entropy_ms": round(t_ent, 3), "idct_ms": round(t_idct, 3), "color_ms": round(t_col, 3),
               "kernels_ms_per_frame": round((t_ent + t_idct + t_col) / n, 4),
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
