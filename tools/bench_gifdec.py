#!/usr/bin/env python3
"""GIF decoder timings on one MI355X, one JSON line per input; every input is one .gif of 80 frames of 512 x 512:

  * pil_noise     PIL-written, noise-like RGB frames (a palette per frame, short LZW strings, the table fills and clears many times a frame)
  * pil_masks     PIL-written, lines and discs on black (delta rectangles with transparency, long strings)
  * own_gif       the project's own .gif (video_out.encode_gif_frames / write_gif) of the same mask-like frames: one palette, strip-wise streams

Per input: device time of the two launches by HIP events (unlzw, compose) on operands that are already on the device; and end to end on the
same box, alternating, host clock around work that ends in a synchronise: file -> (1, 3, L, H, W) fp32 pose tensor on the device through the
decoder (read_frames_device -> pose_tensor_device) against the host route (read_frames -> pose_tensor -> .to(device)).  Both routes give the same
tensor; the line says whether they did.

    python tools/bench_gifdec.py [--frames 80] [--reps 20] [--pairs 7] [--out FILE]     (default: rewrites profiles/gifdec/bench_gifdec.jsonl)"""
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

from tools.bench_pngdec import mask_clip, noise_clip, timed  # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--frames", type=int, default=80)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--pairs", type=int, default=7)
    p.add_argument("--out", type=str, default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "gifdec",
                                                           "bench_gifdec.jsonl"))
    a = p.parse_args()
    from PIL import Image
    from mmgt_amd import hip, inputs, video_in, video_out
    dev = torch.device("cuda:0")
    n, H, W = a.frames, 512, 512
    tmp = tempfile.mkdtemp(prefix="bench_gifdec_")
    paths = {}
    for name, frames in (("pil_noise", noise_clip(n, H, W)), ("pil_masks", mask_clip(n, H, W))):
        paths[name] = os.path.join(tmp, name + ".gif")
        pil = [Image.fromarray(f) for f in frames]
        pil[0].save(paths[name], save_all=True, append_images=pil[1:], duration=40, loop=0)
    paths["own_gif"] = os.path.join(tmp, "own.gif")
    palette, blobs = video_out.encode_gif_frames(torch.from_numpy(mask_clip(n, H, W)).to(dev))
    video_out.write_gif(paths["own_gif"], palette, blobs, W, H, 25)
    lines = []
    for name, path in paths.items():
        h = video_in.parse_gif(open(path, "rb").read())
        tab, pal, data, chunks = video_in.gif_operands(h)
        assert len(chunks) == 1 and len(tab) == n
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
        d_data, d_tab, d_pal = up(data.copy()), up(tab), up(pal)
        idx, status = hip.gif_unlzw(d_data, d_tab, chunks[0][2])
        carry = torch.empty((2, H, W, 3), device=dev, dtype=torch.uint8)
        out = hip.gif_compose(d_tab, idx, d_pal, carry, H, W)
        assert not bool(status.any())
        lib, st = hip.lib(), torch.cuda.current_stream().cuda_stream
        t_lzw = timed(lambda: lib.mmgt_gif_unlzw(d_data.data_ptr(), d_data.numel(), d_tab.data_ptr(), idx.data_ptr(), idx.numel(), status.data_ptr(),
                                                 n, st), a.reps)
        t_cmp = timed(lambda: lib.mmgt_gif_compose(d_tab.data_ptr(), idx.data_ptr(), idx.numel(), d_pal.data_ptr(), carry.data_ptr(), out.data_ptr(),
                                                   n, H, W, st), a.reps)

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
        rec = {"input": name, "frames": n, "size": [H, W], "bytes_lzw": int(tab[-1, 6]), "indices": int(chunks[0][2]),
               "sub_rectangles": int(sum(1 for f in h.frames if (f.width, f.height) != (W, H))), "box": torch.cuda.get_device_name(0),
               "device_equals_host_route": same, "unlzw_ms": round(t_lzw, 3), "compose_ms": round(t_cmp, 3),
               "kernels_ms_per_frame": round((t_lzw + t_cmp) / n, 4),
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
