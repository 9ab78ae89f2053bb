#!/usr/bin/env python3
"""Device image resize timings on one MI355X, one JSON line per input:

  * pose_1080p_to_512   80 frames of 1920 x 1080 -> 512 x 512, bilinear (transforms.Resize of the pose clip)
  * photo_to_vae_clip   one 1024 x 1536 photo -> 512 x 512 Lanczos (the VAE's input) and -> 224 x 224 bicubic (CLIP's)

Per input: device time of each launch by HIP events (the horizontal and the vertical pass are called on their own through the C ABI, on operands
that are already on the device), the bytes each launch reads and writes once and what that is per second, beside the HBM copy rate of the part
(8.0 TB/s by specification, 6.29 TB/s measured with a float4 copy); and end to end on the same box, alternating, host clock around work that ends
in a synchronise: frames on the device -> the fp32 tensors on the device, against PIL on the host -> .to(device).  The line says whether the two
routes gave the same tensors.

    python tools/bench_resize.py [--frames 80] [--reps 20] [--pairs 7] [--out FILE]     (default: rewrites profiles/resize/bench_resize.jsonl)"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBS_SPEC, HBM_TBS_COPY = 8.0, 6.29


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


def picture(n, H, W):
    """Seeded frames with the statistics of a rendered pose clip: smooth colour fields, a few hard-edged bright strokes, mild noise."""
    rng = np.random.default_rng(20261019)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    base = np.stack([96 + 70 * np.sin(0.013 * (c + 1) * xx) * np.cos(0.011 * yy + c) for c in range(3)], axis=-1)
    out = np.empty((n, H, W, 3), np.uint8)
    for k in range(n):
        f = np.roll(base, 7 * k, axis=1).copy()
        for s in range(6):
            cx, cy = rng.uniform(0, W), rng.uniform(0, H)
            f[(np.abs(xx - cx) < 4 + s) & (np.abs(yy - cy) < 60)] = rng.uniform(120, 255, 3)
        out[k] = np.clip(f + rng.normal(0, 3, f.shape), 0, 255).astype(np.uint8)
    return out


def launches(x, Hd, Wd, filt, lut, reps):
    """(ms, bytes) of the horizontal and of the vertical launch of x (n, Hs, Ws, 3) -> Hd x Wd, each called alone; the vertical one has the epilogue."""
    from mmgt_amd import conditioning as C, hip
    n, Hs, Ws, c = x.shape
    tx, ty = C.resample_tables_device(Ws, Wd, filt, x.device), C.resample_tables_device(Hs, Hd, filt, x.device)
    mid = torch.empty((n, Hs, Wd, c), dtype=torch.uint8, device=x.device)
    out = torch.empty((c, n, Hd, Wd), dtype=torch.float32, device=x.device)
    lib, st = hip.lib(), torch.cuda.current_stream().cuda_stream                  # the C entry itself: no Python between two launches but this call
    t_h = timed(lambda: lib.mmgt_resize_u8(x.data_ptr(), None, mid.data_ptr(), None, None, n, Hs, Ws, Hs, Wd, c, tx[0].data_ptr(), tx[1].data_ptr(),
                                           tx[1].shape[1], None, None, 0, st), reps)
    t_v = timed(lambda: lib.mmgt_resize_u8(mid.data_ptr(), None, None, out.data_ptr(), lut.data_ptr(), n, Hs, Wd, Hd, Wd, c, None, None, 0,
                                           ty[0].data_ptr(), ty[1].data_ptr(), ty[1].shape[1], st), reps)
    rate = lambda b, ms: round(b / ms / 1e9, 3)                                    # TB/s
    bh, bv = x.numel() + mid.numel(), mid.numel() + 4 * out.numel()
    return {"h_ms": round(t_h, 4), "h_bytes": bh, "h_tbs": rate(bh, t_h), "v_ms": round(t_v, 4), "v_bytes": bv, "v_tbs": rate(bv, t_v),
            "taps": [int(tx[1].shape[1]), int(ty[1].shape[1])]}


def alternate(dev_fn, host_fn, pairs):
    dev_s, host_s = [], []
    for _ in range(pairs):
        for f, acc in ((dev_fn, dev_s), (host_fn, host_s)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            acc.append(time.perf_counter() - t0)
    return dev_s, host_s


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--frames", type=int, default=80)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--pairs", type=int, default=7)
    p.add_argument("--out", type=str, default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "resize",
                                                           "bench_resize.jsonl"))
    a = p.parse_args()
    from PIL import Image
    from transformers import CLIPImageProcessor
    from mmgt_amd import inputs
    from mmgt_amd.pipeline import _pil_to_tensor
    dev = torch.device("cuda:0")
    med = lambda v: sorted(v)[len(v) // 2]
    ms = lambda v: [round(1e3 * t, 2) for t in v]
    common = {"box": torch.cuda.get_device_name(0), "hbm_tbs_spec": HBM_TBS_SPEC, "hbm_tbs_copy_measured": HBM_TBS_COPY}
    lines = []

    # ---- the pose clip
    n = a.frames
    clip = picture(n, 1080, 1920)
    x = torch.from_numpy(clip).to(dev)
    pil = [Image.fromarray(f) for f in clip]
    unit = (torch.arange(256, dtype=torch.float32) / 255.0).repeat(3, 1).to(dev)
    device_route = lambda: inputs.pose_tensor_device(x, 512, 512, resize=True)
    host_route = lambda: inputs.pose_tensor(pil, 512, 512).to(dev)
    same = bool(torch.equal(device_route(), host_route()))                                     # also warms both
    dev_s, host_s = alternate(device_route, host_route, a.pairs)
    rec = {"input": "pose_1080p_to_512", "frames": n, "from": [1080, 1920], "to": [512, 512], "filter": "bilinear", **common,
           "device_equals_host_route": same, **launches(x, 512, 512, "bilinear", unit, a.reps),
           "device_route_ms": ms(dev_s), "host_route_ms": ms(host_s),
           "device_route_ms_per_frame_median": round(1e3 * med(dev_s) / n, 4), "host_route_ms_per_frame_median": round(1e3 * med(host_s) / n, 4)}
    print(json.dumps(rec), flush=True)
    lines.append(json.dumps(rec))
    del x, clip, pil

    # ---- the reference photo
    photo = picture(1, 1536, 1024)[0]
    y = torch.from_numpy(photo).to(dev)
    img = Image.fromarray(photo)
    proc = CLIPImageProcessor()
    device_route = lambda: inputs.ref_image_tensors_device(y, 512, 512)

    def host_route():
        return (_pil_to_tensor(img, 512, 512, True)[None].to(dev), proc.preprocess(img.resize((224, 224)), return_tensors="pt").pixel_values.to(dev))
    d, h = device_route(), host_route()
    same = [bool(torch.equal(d[0], h[0])), bool(torch.equal(d[1], h[1]))]
    dev_s, host_s = alternate(device_route, host_route, a.pairs)
    lut = torch.zeros((3, 256), device=dev)
    rec = {"input": "photo_to_vae_clip", "from": [1536, 1024], **common, "vae_equals_host_route": same[0], "clip_equals_host_route": same[1],
           "lanczos_512": launches(y[None], 512, 512, "lanczos", lut, a.reps), "bicubic_224": launches(y[None], 224, 224, "bicubic", lut, a.reps),
           "device_route_ms": ms(dev_s), "host_route_ms": ms(host_s),
           "device_route_ms_median": round(1e3 * med(dev_s), 3), "host_route_ms_median": round(1e3 * med(host_s), 3)}
    print(json.dumps(rec), flush=True)
    lines.append(json.dumps(rec))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
