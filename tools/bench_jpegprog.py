#!/usr/bin/env python3
"""Progressive JPEG decoder timings on one MI355X, one JSON line per input; the files are PIL-written at quality 90, 4:2:0, with PIL's
ten-scan script and no restart markers, so a frame is decoded by five lanes in the first level's launch, four in the second and one in the third:

  * frames_24x512      24 frames of 512 x 512 with the statistics of a rendered pose clip
  * photo_1x1024       one 1024 x 1024 photograph-like image (smooth fields, edges, texture, sensor noise)

Per input: device time by HIP events of each level's launch (the first with its zero fill) and of the idct and colour launches, on operands that
are already on the device; and end to end on the same box, alternating, host clock around work that ends in a synchronise: file bytes -> (n, H, W,
3) uint8 on the device, for the progressive files through decode_jpeg_frames(progressive=True), for their baseline twins (the same arrays, quality
and subsampling) through the existing device path, and for the progressive files through the PIL route (host decode + upload).  All three give the
same tensor when PIL is built on libjpeg-turbo; the line says whether they did.

    python tools/bench_jpegprog.py [--reps 10] [--pairs 7] [--out FILE]     (default: rewrites profiles/jpegprog/bench_jpegprog.jsonl)"""
import argparse
import io
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_jpegdec import clip, timed  # noqa: E402


def photo(H, W):
    """A seeded photograph-like image: large smooth fields, a few hard edges, band-limited texture and mild sensor noise."""
    rng = np.random.default_rng(20261020)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    f = np.stack([110 + 60 * np.sin(0.004 * (c + 1) * xx + c) * np.cos(0.003 * yy + 0.5 * c) for c in range(3)], axis=-1)
    for _ in range(12):
        cx, cy, r = rng.uniform(0, W), rng.uniform(0, H), rng.uniform(30, 200)
        f[(xx - cx) ** 2 + (yy - cy) ** 2 < r * r] += rng.uniform(-50, 50, 3)
    f += (12 * np.sin(0.35 * xx + 0.2 * yy) * np.sin(0.05 * yy))[..., None]
    return np.clip(f + rng.normal(0, 4, f.shape), 0, 255).astype(np.uint8)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--pairs", type=int, default=7)
    p.add_argument("--quality", type=int, default=90)
    p.add_argument("--out", type=str, default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "jpegprog",
                                                           "bench_jpegprog.jsonl"))
    a = p.parse_args()
    from PIL import Image, features
    from mmgt_amd import hip, video_in
    dev = torch.device("cuda:0")

    def jpeg(frame, **kw):
        buf = io.BytesIO()
        Image.fromarray(frame).save(buf, format="JPEG", quality=a.quality, subsampling=2, **kw)
        return buf.getvalue()

    lines = []
    for name, frames in (("frames_24x512", clip(24, 512, 512)), ("photo_1x1024", photo(1024, 1024)[None])):
        n, H, W = frames.shape[:3]
        prog, base = [jpeg(f, progressive=True) for f in frames], [jpeg(f) for f in frames]
        heads = [video_in.parse_jpeg(j, progressive=True) for j in prog]
        ops = video_in.prog_batch_operands(prog, heads)
        geo = heads[0].geometry
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
        d = {k: up(ops[k].copy()) for k in ("data", "offsets", "seginfo", "scaninfo", "huff", "tables")}
        fb, _ = hip.jpegdec_sizes(*geo)
        coef = torch.empty((n, fb, 64), device=dev, dtype=torch.int16)
        status = torch.empty((len(ops["seginfo"]),), device=dev, dtype=torch.int32)
        lv = ops["levels"].tolist()

        def level(k):
            x, y = lv[k], lv[k + 1]
            hip.jpegprog_entropy(d["data"], d["offsets"][x:y + 1], d["seginfo"][x:y], d["scaninfo"], d["huff"], coef, status[x:y], *geo, zero_fill=k == 0)

        def all_levels():
            for k in range(len(lv) - 1):
                level(k)
        # a level's launch refines what the lower levels left (and would read its own output as history if repeated on it), so every repetition
        # runs the lower levels afresh, untimed, and the events bracket the one launch
        def time_level(k, warm=2):
            total, e0, e1 = 0.0, torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for rep in range(warm + a.reps):
                for j in range(k):
                    level(j)
                e0.record()
                level(k)
                e1.record()
                torch.cuda.synchronize()
                total += e0.elapsed_time(e1) if rep >= warm else 0.0
            return total / a.reps

        t_levels = [time_level(k) for k in range(len(lv) - 1)]
        assert int(status.abs().sum()) == 0
        all_levels()
        planes = hip.jpegdec_idct(coef, d["tables"], *geo)
        out = hip.jpegdec_color(planes, *geo)
        lib, st = hip.lib(), torch.cuda.current_stream().cuda_stream
        t_idct = timed(lambda: lib.mmgt_jpegdec_idct(coef.data_ptr(), d["tables"].data_ptr(), planes.data_ptr(), n, *geo, st), a.reps)
        t_col = timed(lambda: lib.mmgt_jpegdec_color(planes.data_ptr(), out.data_ptr(), n, *geo, st), a.reps)

        routes = {"progressive_device": lambda: video_in.decode_jpeg_frames(prog, dev, progressive=True),
                  "baseline_twin_device": lambda: video_in.decode_jpeg_frames(base, dev),
                  "progressive_pil": lambda: torch.from_numpy(np.stack([np.asarray(Image.open(io.BytesIO(j)).convert("RGB")) for j in prog])).to(dev)}
        first = {k: f() for k, f in routes.items()}                                             # also warms every route
        same = bool(torch.equal(first["progressive_device"], first["baseline_twin_device"]) and
                    torch.equal(first["progressive_device"], first["progressive_pil"]))
        times = {k: [] for k in routes}
        for _ in range(a.pairs):
            for k, f in routes.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()
                torch.cuda.synchronize()
                times[k].append(time.perf_counter() - t0)
        med = lambda v: sorted(v)[len(v) // 2]
        rec = {"input": name, "frames": n, "size": [H, W], "subsampling": "4:2:0", "quality": a.quality, "scans_per_frame": len(heads[0].scans),
               "lanes_per_level": [lv[k + 1] - lv[k] for k in range(len(lv) - 1)], "bytes_in": int(ops["data"].size),
               "baseline_twin_bytes": sum(len(j) for j in base), "box": torch.cuda.get_device_name(0),
               "pil_libjpeg_turbo": bool(features.check_feature("libjpeg_turbo")), "all_routes_equal": same,
               "level_ms": [round(t, 3) for t in t_levels], "idct_ms": round(t_idct, 3), "color_ms": round(t_col, 3),
               "kernels_ms_per_frame": round((sum(t_levels) + t_idct + t_col) / n, 4)}
        for k, v in times.items():
            rec[k + "_ms"] = [round(1e3 * t, 2) for t in v]
            rec[k + "_ms_per_frame_median"] = round(1e3 * med(v) / n, 3)
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
