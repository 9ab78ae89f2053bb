#!/usr/bin/env python3
"""WebP lossless decoder timings on one MI355X, one JSON line per input; every input is one animated .webp of 80 frames of 512 x 512:

  * pil_noise     VAE-like noise saved by PIL at method 0: nearly all-literal streams, one prefix-code group
  * pil_masks     white shapes on black saved by PIL at method 4: many prefix-code groups, far distances, a colour cache
  * own_masks     the project's own .webp (video_out.encode_webp_frames / write_webp) of the same mask frames: one group, distance-1 copies
  * pil_pose      lines and discs on black, as pose frames have them, saved by PIL at its default method

Per input: device time of the three launches by HIP events (decode, untransform, compose) on operands that are already on the device -- the
untransform launch uses its input up, so its repeats run on words it has already undone, which costs the same; and end to end on the same box,
alternating, host clock around work that ends in a synchronise: file -> (1, 3, L, H, W) fp32 pose tensor on the device through the decoder
(read_frames_device -> pose_tensor_device) against the host route (read_frames -> pose_tensor -> .to(device)).  Both routes give the same tensor;
the line says whether they did.

    python tools/bench_webpdec.py [--frames 80] [--reps 10] [--pairs 5] [--out FILE]     (default: rewrites profiles/webpdec/bench_webpdec.jsonl)"""
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_pngdec import mask_clip as pose_clip, noise_clip, timed  # noqa: E402


def shapes_clip(n, H, W):
    """White discs and bars on black, as a hands or face mask has them."""
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.zeros((n, H, W, 3), np.uint8)
    for f in range(n):
        out[f][(yy - H * 0.4 - f) ** 2 * 4 + (xx - W * 0.5) ** 2 < (min(H, W) * 0.3) ** 2] = 255
        out[f][(yy > H * 0.7) & (abs(xx - W * 0.3 - 2 * f) < W * 0.12)] = 255
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--frames", type=int, default=80)
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--pairs", type=int, default=5)
    p.add_argument("--out", type=str, default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "webpdec",
                                                           "bench_webpdec.jsonl"))
    a = p.parse_args()
    from PIL import Image
    from mmgt_amd import hip, inputs, video_in, video_out
    dev = torch.device("cuda:0")
    n, H, W = a.frames, 512, 512
    tmp = tempfile.mkdtemp(prefix="bench_webpdec_")
    paths = {}
    for name, frames, method in (("pil_noise", noise_clip(n, H, W), 0), ("pil_masks", shapes_clip(n, H, W), 4), ("pil_pose", pose_clip(n, H, W), None)):
        paths[name] = os.path.join(tmp, name + ".webp")
        ims = [Image.fromarray(f) for f in frames]
        ims[0].save(paths[name], format="WEBP", save_all=True, append_images=ims[1:], lossless=True, duration=40,
                    **({} if method is None else {"method": method}))
    paths["own_masks"] = os.path.join(tmp, "own_masks.webp")
    video_out.write_webp(paths["own_masks"], video_out.encode_webp_frames(torch.from_numpy(shapes_clip(n, H, W)).to(dev)), W, H, 25)
    lines = []
    for name in ("pil_noise", "pil_masks", "own_masks", "pil_pose"):
        path = paths[name]
        header = video_in.parse_webp(open(path, "rb").read())
        tab, data, chunks = video_in.webp_operands([header], None, 1 << 40)                   # one set of launches, whatever it takes
        (_, _, scr_words, argb_words), = chunks
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
        d_data, d_tab = up(data.copy()), up(tab)
        scratch = torch.empty((scr_words,), device=dev, dtype=torch.int32)
        carry = torch.empty((H, W), device=dev, dtype=torch.int32)
        st0 = hip.webp_decode(d_data, d_tab, scratch)
        argb, st1 = hip.webp_untransform(d_tab, scratch, argb_words)
        out = hip.webp_compose(d_tab, argb, carry, H, W)
        assert not bool(st0.any()) and not bool(st1.any())
        lib, st = hip.lib(), torch.cuda.current_stream().cuda_stream
        t_dec = timed(lambda: lib.mmgt_webp_decode(d_data.data_ptr(), d_data.numel(), d_tab.data_ptr(), scratch.data_ptr(), scratch.numel(),
                                                   st0.data_ptr(), n, st), a.reps, warm=1)
        t_unt = timed(lambda: lib.mmgt_webp_untransform(d_tab.data_ptr(), scratch.data_ptr(), scratch.numel(), argb.data_ptr(), argb.numel(),
                                                        st1.data_ptr(), n, st), a.reps, warm=1)
        t_com = timed(lambda: lib.mmgt_webp_compose(d_tab.data_ptr(), argb.data_ptr(), argb.numel(), carry.data_ptr(), out.data_ptr(), n, H, W, st),
                      a.reps, warm=1)

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
        rec = {"input": name, "frames": n, "size": [H, W], "bytes_in": int(sum(len(f.payload) for f in header.frames)),
               "full_canvas_frames": int(sum((f.width, f.height) == (W, H) for f in header.frames)), "key_frames": int(sum(f.key for f in header.frames)),
               "scratch_mib": round(scr_words * 4 / 2 ** 20, 1), "box": torch.cuda.get_device_name(0), "device_equals_host_route": same,
               "decode_ms": round(t_dec, 3), "untransform_ms": round(t_unt, 3), "compose_ms": round(t_com, 3),
               "kernels_ms_per_frame": round((t_dec + t_unt + t_com) / n, 4),
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
