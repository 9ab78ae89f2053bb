#!/usr/bin/env python3
"""Device GIF encoder timings on one MI355X, one JSON line per clip length (24 and 96 frames of 512 x 512 out of a VAE decode with random-init
weights):

  * device time of the stages by HIP events, as ms per frame: histogram, index, lzw, pack, and the copy of the finished bytes to the host;
    the host's palette + lookup table (gif_palette / gif_lut, once per clip) in ms;
  * LZW time and stream size for several strip_rows (the choice of video_out.GIF_STRIP_ROWS), strip_rows = H being one strip per frame with
    no Clear codes at strip boundaries;
  * end to end on the same box, alternating: save_videos_grid(frames, "x.gif") with gif_encoder="pil" (the default branch, the baseline) against
    gif_encoder="device"; host clock, host uint8 frames in, file out;
  * file sizes: device, PIL, device with strip_rows = H;
  * dithering and frame differencing (encode_gif_frames(dither="fs", delta=True)): ms per frame of the mmgt_gif_dither launch beside
    mmgt_gif_index; file bytes for the four combinations on the clip and on one with a static background (static_clip); and the share of that
    background's pixels whose index changes from one frame to the next, with and without dithering: the crawl that eats into what delta saves.

    python tools/bench_gif.py [--reps 20] [--pairs 3] [--out profiles/gif/bench_gif.jsonl]"""
import argparse
import json
import os
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


def static_clip(frames):
    """A clip with a static background: frame 0 everywhere, and a window of a quarter of each side that shows frame k's own pixels and moves along
    the diagonal.  -> (the clip, k -> the window's (y0, x0))."""
    n, H, W, _ = frames.shape

    def box(k):
        return (k * (H - H // 4)) // max(1, n - 1), (k * (W - W // 4)) // max(1, n - 1)

    clip = frames[:1].repeat(n, 1, 1, 1)
    for k in range(n):
        y0, x0 = box(k)
        clip[k, y0:y0 + H // 4, x0:x0 + W // 4] = frames[k, y0:y0 + H // 4, x0:x0 + W // 4]
    return clip.contiguous(), box


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--pairs", type=int, default=3)
    p.add_argument("--frames", type=int, nargs="+", default=[24, 96])
    p.add_argument("--sweep", type=int, nargs="+", default=[4, 8, 16, 32, 64, 512])
    p.add_argument("--out", type=str, default=os.path.join("profiles", "gif", "bench_gif.jsonl"))
    a = p.parse_args()
    from mmgt_amd import hip, video_out
    from mmgt_amd.synthetic import hash_uniform, synth_state_dict
    from mmgt_amd.vae import AutoencoderKL, vae_decoder_spec
    dev = torch.device("cuda:0")
    vae = AutoencoderKL(device=dev, dtype=torch.bfloat16)
    vae.load_state_dict(synth_state_dict(vae_decoder_spec(), prefix="vae.", device=dev))
    lines = []
    tmp = tempfile.mkdtemp(prefix="bench_gif_")
    for n in a.frames:
        lat = hash_uniform("bench.gif.lat", (1, 4, n, 64, 64), 1.7).to(dev)
        frames = vae.decode_video_uint8(lat)[0].contiguous()                              # (n, 512, 512, 3) on the device
        H, W = frames.shape[1:3]
        rows = min(video_out.GIF_STRIP_ROWS, H)
        hist = hip.gif_histogram(frames).cpu().numpy().view(np.uint32)
        t0 = time.perf_counter()
        palette = video_out.gif_palette(hist)
        t1 = time.perf_counter()
        lut_h = video_out.gif_lut(palette)
        t2 = time.perf_counter()
        lut = torch.from_numpy(lut_h).to(dev)
        idx = hip.gif_index(frames, lut)
        lzw = hip.gif_lzw(idx, rows)
        pk = hip.gif_pack(*lzw)
        sizes = pk[1].tolist()
        t_hist = timed(lambda: hip.gif_histogram(frames), a.reps)
        t_idx = timed(lambda: hip.gif_index(frames, lut), a.reps)
        t_lzw = timed(lambda: hip.gif_lzw(idx, rows, out=lzw), a.reps)
        t_pack = timed(lambda: hip.gif_pack(*lzw, out=pk), a.reps)
        t_copy = timed(lambda: pk[0][:, :max(sizes)].cpu(), a.reps)
        sweep = []
        for r in a.sweep:
            r = min(r, H)
            o = hip.gif_lzw(idx, r)
            sweep.append({"strip_rows": r, "workgroups": int(o[1].numel()), "lzw_ms": round(timed(lambda: hip.gif_lzw(idx, r, out=o), max(3, a.reps // 4)), 3),
                          "stream_bytes": int((o[1].sum(1) + 7).div(8, rounding_mode="floor").sum())})
        rec = {"frames": n, "size": [H, W], "strip_rows": rows, "box": torch.cuda.get_device_name(0), "occupied_bins": int((hist > 0).sum()),
               "histogram_ms_per_frame": round(t_hist / n, 4), "index_ms_per_frame": round(t_idx / n, 4), "lzw_ms_per_frame": round(t_lzw / n, 4),
               "pack_ms_per_frame": round(t_pack / n, 4), "copy_ms_per_frame": round(t_copy / n, 4),
               "palette_host_ms": round(1e3 * (t1 - t0), 1), "lut_host_ms": round(1e3 * (t2 - t1), 1), "strip_rows_sweep": sweep,
               "bytes_raw": int(frames.numel())}
        # end to end, alternating the two writers; host frames in (what save_videos_grid is handed), file out
        host = frames.cpu()[None]
        paths = {k: os.path.join(tmp, f"{k}_{n}.gif") for k in ("pil", "device", "device_one_strip")}
        acc = {"pil": [], "device": []}
        video_out.save_videos_grid(host, paths["device"], fps=25, gif_encoder="device")          # warm
        for _ in range(a.pairs):
            for k in ("pil", "device"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                video_out.save_videos_grid(host, paths[k], fps=25, gif_encoder=k)
                torch.cuda.synchronize()
                acc[k].append(time.perf_counter() - t0)
        pal1, blobs1 = video_out.encode_gif_frames(frames, strip_rows=H)
        video_out.write_gif(paths["device_one_strip"], pal1, blobs1, W, H, 25)
        for k in acc:
            rec[f"save_gif_{k}_ms"] = [round(1e3 * t, 1) for t in acc[k]]
            rec[f"save_gif_{k}_ms_median"] = round(1e3 * sorted(acc[k])[len(acc[k]) // 2], 1)
        for k, path in paths.items():
            rec[f"file_bytes_{k}"] = os.path.getsize(path)
            os.remove(path)
        rec["strip_clear_cost"] = round(rec["file_bytes_device"] / rec["file_bytes_device_one_strip"] - 1, 5)
        # dithering and frame differencing: the dither launch beside mmgt_gif_index, then file bytes for the four combinations on this clip and on
        # one with a static background, and the crawl of error diffusion over that background (nothing here is gated)
        pal_d = torch.from_numpy(palette).to(dev)
        dith = torch.empty_like(idx)
        scratch = torch.empty((max(4, hip.gif_dither_scratch_bytes(n, H, W)),), device=dev, dtype=torch.uint8)
        rec["dither_ms_per_frame"] = round(timed(lambda: hip.gif_dither(frames, lut, pal_d, out=dith, scratch=scratch), max(3, a.reps // 4)) / n, 4)
        rec["dither_band_rows"] = hip.gif_dither_band()
        still, box = static_clip(frames)
        for name, clip in (("", frames), ("_static", still)):
            for dither in (None, "fs"):
                for delta in (False, True):
                    pal2, blobs2 = video_out.encode_gif_frames(clip, dither=dither, delta=delta)
                    path = os.path.join(tmp, "opt.gif")
                    key = f"file_bytes{name}" + ("_fs" if dither else "") + ("_delta" if delta else "")
                    rec[key] = video_out.write_gif(path, pal2, blobs2, W, H, 25, transparent=255 if delta else None)
                    os.remove(path)
        pal_s = video_out.gif_palette(hip.gif_histogram(still).cpu().numpy().view(np.uint32), 255)
        lut_s = torch.from_numpy(video_out.gif_lut(pal_s, 255)).to(dev)
        outside = torch.ones((n - 1, H, W), device=dev, dtype=torch.bool)                     # of frame k + 1: not under the window of frame k or k + 1
        for k in range(n - 1):
            for y0, x0 in (box(k), box(k + 1)):
                outside[k, y0:y0 + H // 4, x0:x0 + W // 4] = False
        for key, m in (("fs", hip.gif_dither(still, lut_s, torch.from_numpy(pal_s).to(dev))), ("plain", hip.gif_index(still, lut_s))):
            rec[f"static_region_changed_share_{key}"] = round(float(((m[1:] != m[:-1]) & outside).sum() / outside.sum()), 5)
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
    os.rmdir(tmp)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
