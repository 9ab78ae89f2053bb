#!/usr/bin/env python3
"""Lossy WebP (VP8 key frame) decoder timings on one MI355X, one JSON line per input; every input is one animated lossy .webp of 80
frames of 512 x 512, of three kinds of content (noise-like, smooth, pose-like: lines and discs on black), each written twice:

  * pil_<kind>    PIL's save_all at quality 75: one token partition, segments, 4 x 4 modes, probability updates, sub-rectangle frames
  * own_<kind>    the project's own writer (video_out.encode_vp8_frames) at quality 75 and 8 token partitions: 16 x 16 modes only

PIL's writer drops a frame that differs too little from the one before, so a PIL file may hold fewer than 80 frames; every count and every
per-frame figure is of the frames the file holds.  A PIL file that carries ALPH chunks (PIL writes them on mask-like clips) is outside the
device decoder's scope; its line says so and times nothing.

Per input: device time of the four launches by HIP events (parse, reconstruct, filter, output) and of the compose launch on operands that are
already on the device; and end to end on the same box, alternating, host clock around work that ends in a synchronise: file -> (1, 3, L, H, W)
fp32 pose tensor on the device through the decoder (read_frames_device(webp_lossy=True) -> pose_tensor_device) against the host route
(read_frames -> pose_tensor -> .to(device)).  Both routes give the same tensor; the line says whether they did.

    python tools/bench_vp8dec.py [--frames 80] [--reps 10] [--pairs 5] [--out FILE]     (default: rewrites profiles/vp8dec/bench_vp8dec.jsonl)"""
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


def smooth_clip(n, H, W):
    """Slow colour ramps that drift from frame to frame."""
    yy, xx = np.mgrid[0:H, 0:W]
    return np.stack([np.stack([64 + ((xx + 3 * f) * 160) // W, 32 + (yy * 190) // H, 128 + ((xx + yy + 2 * f) * 100) // (W + H)], -1).astype(np.uint8)
                     for f in range(n)])


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--frames", type=int, default=80)
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--pairs", type=int, default=5)
    p.add_argument("--inputs", type=str, default="", help="comma-separated input names (default: all six)")
    p.add_argument("--out", type=str, default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "vp8dec",
                                                           "bench_vp8dec.jsonl"))
    a = p.parse_args()
    from PIL import Image
    from mmgt_amd import hip, inputs, video_in, video_out
    dev = torch.device("cuda:0")
    n, H, W = a.frames, 512, 512
    tmp = tempfile.mkdtemp(prefix="bench_vp8dec_")
    paths = {}
    for kind, frames in (("noise", noise_clip(n, H, W)), ("smooth", smooth_clip(n, H, W)), ("pose", pose_clip(n, H, W))):
        frames = np.ascontiguousarray(frames if frames.ndim == 4 else np.repeat(frames[..., None], 3, -1))
        paths["pil_" + kind] = os.path.join(tmp, f"pil_{kind}.webp")
        ims = [Image.fromarray(f) for f in frames]
        ims[0].save(paths["pil_" + kind], format="WEBP", save_all=True, append_images=ims[1:], quality=75, duration=40)
        paths["own_" + kind] = os.path.join(tmp, f"own_{kind}.webp")
        video_out.write_webp(paths["own_" + kind], video_out.encode_vp8_frames(torch.from_numpy(frames).to(dev), 75, partitions=8), W, H, 25, lossy=True)
    lines = []
    for name in sorted(paths) if not a.inputs else a.inputs.split(","):
        path = paths[name]
        try:
            header = video_in.parse_webp(open(path, "rb").read(), lossy=True)
        except ValueError as e:
            rec = {"input": name, "frames": n, "size": [H, W], "refused": str(e)[:120]}
            print(json.dumps(rec), flush=True)
            lines.append(json.dumps(rec))
            continue
        tab, ltab, vtab, lidx, vidx, data, chunks = video_in.webp_operands_lossy([header], None, 1 << 40)   # one set of launches, whatever it takes
        (_, _, _, _, _, _, scr_words, argb_words), = chunks
        nf = len(tab)                                                                           # PIL drops frames that differ too little from the one before
        assert len(ltab) == 0 and len(vtab) == nf == len(header.frames) <= n
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
        d_data, d_tab, d_vtab = up(data.copy()), up(tab), up(vtab)
        scratch = torch.empty((scr_words,), device=dev, dtype=torch.int32)
        argb = torch.empty((argb_words,), device=dev, dtype=torch.int32)
        carry = torch.empty((H, W), device=dev, dtype=torch.int32)
        biggest = int((vtab[:, 5] * vtab[:, 6]).max())
        st = [hip.vp8dec_parse(d_data, d_vtab, scratch), hip.vp8dec_reconstruct(d_vtab, scratch), hip.vp8dec_filter(d_vtab, scratch),
              hip.vp8dec_output(d_vtab, scratch, argb, biggest)]
        out = hip.webp_compose(d_tab, argb, carry, H, W)
        assert not any(bool(s.any()) for s in st)
        assert tuple(out.shape) == (nf, H, W, 3)
        lib, cs, nv = hip.lib(), torch.cuda.current_stream().cuda_stream, nf
        sp, ss = scratch.data_ptr(), scratch.numel()
        t_par = timed(lambda: lib.mmgt_vp8dec_parse(d_data.data_ptr(), d_data.numel(), d_vtab.data_ptr(), sp, ss, st[0].data_ptr(), nv, cs), a.reps, warm=1)
        t_rec = timed(lambda: lib.mmgt_vp8dec_reconstruct(d_vtab.data_ptr(), sp, ss, st[1].data_ptr(), nv, cs), a.reps, warm=1)
        # the filter works in place: its repeats filter planes that are filtered already, which costs the same edges and the same tests
        t_fil = timed(lambda: lib.mmgt_vp8dec_filter(d_vtab.data_ptr(), sp, ss, st[2].data_ptr(), nv, cs), a.reps, warm=1)
        t_out = timed(lambda: lib.mmgt_vp8dec_output(d_vtab.data_ptr(), sp, ss, argb.data_ptr(), argb.numel(), st[3].data_ptr(), nv, biggest, cs), a.reps,
                      warm=1)
        t_com = timed(lambda: lib.mmgt_webp_compose(d_tab.data_ptr(), argb.data_ptr(), argb.numel(), carry.data_ptr(), out.data_ptr(), nf, H, W, cs),
                      a.reps, warm=1)

        def device_route():
            return inputs.pose_tensor_device(video_in.read_frames_device(path, n, dev, webp_lossy=True), W, H)

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
        rec = {"input": name, "frames": nf, "size": [H, W], "bytes_in": int(sum(len(f.payload) for f in header.frames)),
               "full_canvas_frames": int(sum((f.width, f.height) == (W, H) for f in header.frames)),
               "scratch_mib": round(scr_words * 4 / 2 ** 20, 1), "box": torch.cuda.get_device_name(0), "device_equals_host_route": same,
               "parse_ms": round(t_par, 3), "reconstruct_ms": round(t_rec, 3), "filter_ms": round(t_fil, 3), "output_ms": round(t_out, 3),
               "compose_ms": round(t_com, 3), "kernels_ms_per_frame": round((t_par + t_rec + t_fil + t_out + t_com) / nf, 4),
               "device_route_ms": [round(1e3 * t, 2) for t in dev_s], "host_route_ms": [round(1e3 * t, 2) for t in host_s],
               "device_route_ms_per_frame_median": round(1e3 * med(dev_s) / nf, 3), "host_route_ms_per_frame_median": round(1e3 * med(host_s) / nf, 3)}
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
    shutil.rmtree(tmp, ignore_errors=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
