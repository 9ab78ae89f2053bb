#!/usr/bin/env python3
"""Device WebP lossless encoder on one MI355X, one JSON line per input kind (24 frames of 512 x 512): `vae` out of a VAE decode with random-init
weights (close to noise; the input of tools/bench_png.py), `smooth` (ramps and soft shading), `mask` (flat white shapes on black) and `pose` (the
rasteriser's pose frames, csrc/dwpose.hip):

  * file sizes: the VP8L payloads of this writer, this project's PNG streams (encode_png_frames) and PIL's save(format="WEBP", lossless=True) at
    methods 0 and 4, all on the same frames (PIL on the first --pil-frames of them, with this writer's bytes for the same frames beside it);
  * on `vae`: device time of the stages by HIP events, as ms per frame: predict, histogram, coding (with the upload of its tables), pack, and
    the copy of the finished bytes to the host; the host's code building (webp_frame_tables + webp_frame_header per frame) in ms per frame;
  * on `vae` and `pose`: histogram + coding time, host tables time and payload bytes for several strip_rows (the choice of
    video_out.WEBP_STRIP_ROWS), strip_rows = H being one strip per frame;
  * on `vae`: end to end on the same box, alternating: save_videos_grid(frames, "x.webp") against PIL's animated
    Image.save(format="WEBP", lossless=True, method=0, save_all=True) of the same host frames; host clock, host uint8 frames in, file out.

    python tools/bench_webp.py [--reps 20] [--pairs 3] [--out profiles/webp/bench_webp.jsonl]"""
import argparse
import io
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


def tables(hist, modes, W, H, video_out):
    k, strips = hist.shape[:2]
    codes, heads, want = np.empty((k, 792), np.uint32), [], np.empty((k, 1 + strips), np.int64)
    for f in range(k):
        codes[f], cost, described = video_out.webp_frame_tables(hist[f].sum(0))
        head, want[f, 0] = video_out.webp_frame_header(W, H, modes[f], described)
        heads.append(head)
        want[f, 1:] = hist[f] @ cost
    return codes, heads, want


def smooth_clip(n, H, W, dev):
    y, x = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    out = []
    for f in range(n):
        r = 128 + 100 * torch.sin((x + 3 * f) / 61) * torch.cos(y / 47)
        g = 0.3 * x + 0.2 * y + 2 * f
        b = 128 + 90 * torch.cos((x + y) / 83 + 0.1 * f)
        out.append(torch.stack([r, g, b], -1).clamp(0, 255).to(torch.uint8))
    return torch.stack(out).contiguous()


def mask_clip(n, H, W, dev):
    y, x = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    out = torch.zeros((n, H, W, 3), device=dev, dtype=torch.uint8)
    for f in range(n):
        out[f][((y - 0.4 * H - f) ** 2 * 4 + (x - 0.5 * W) ** 2 < (0.3 * min(H, W)) ** 2) | ((y > 0.7 * H) & ((x - 0.3 * W - 2 * f).abs() < 0.12 * W))] = 255
    return out


def pose_clip(n, dev, hip):
    """A skeleton that drifts from frame to frame, every point visible, through the rasteriser."""
    rng = np.random.default_rng(7)
    base = rng.normal(0, 0.12, (1, 134, 2)) + np.array([-0.2, -0.2])
    kp = np.zeros((n, 134, 3), np.float32)
    kp[..., :2] = base + 0.004 * np.arange(n)[:, None, None] + rng.normal(0, 0.003, (n, 134, 2))
    kp[..., 2] = 0.5
    return hip.dwpose_draw(torch.from_numpy(kp).to(dev))[0].contiguous()


def pil_webp_bytes(frames, method):
    from PIL import Image
    total = 0
    for f in frames:
        buf = io.BytesIO()
        Image.fromarray(f).save(buf, format="WEBP", lossless=True, method=method)
        total += buf.tell() - 20                                                        # RIFF, size, WEBP, VP8L, size
    return total


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--pairs", type=int, default=3)
    p.add_argument("--frames", type=int, default=24)
    p.add_argument("--pil-frames", type=int, default=4)
    p.add_argument("--sweep", type=int, nargs="+", default=[4, 8, 16, 32, 64, 128, 512])
    p.add_argument("--out", type=str, default=os.path.join("profiles", "webp", "bench_webp.jsonl"))
    a = p.parse_args()
    from PIL import Image
    from mmgt_amd import hip, video_out
    from mmgt_amd.synthetic import hash_uniform, synth_state_dict
    from mmgt_amd.vae import AutoencoderKL, vae_decoder_spec
    dev = torch.device("cuda:0")
    vae = AutoencoderKL(device=dev, dtype=torch.bfloat16)
    vae.load_state_dict(synth_state_dict(vae_decoder_spec(), prefix="vae.", device=dev))
    n = a.frames
    lat = hash_uniform("bench.gif.lat", (1, 4, n, 64, 64), 1.7).to(dev)
    clips = {"vae": vae.decode_video_uint8(lat)[0].contiguous(), "smooth": smooth_clip(n, 512, 512, dev), "mask": mask_clip(n, 512, 512, dev),
             "pose": pose_clip(n, dev, hip)}
    lines = []
    tmp = tempfile.mkdtemp(prefix="bench_webp_")
    for kind, frames in clips.items():
        H, W = frames.shape[1:3]
        rows = min(video_out.WEBP_STRIP_ROWS, H)
        po = hip.webp_predict(frames)
        data = po[1].view(n, H * W)
        modes = po[0].cpu().numpy()

        def stages(r):
            hist = hip.webp_histogram(data, r * W)
            h = hist.cpu().numpy().view(np.uint32).astype(np.int64)
            t0 = time.perf_counter()
            tb = tables(h, modes, W, H, video_out)
            host_ms = 1e3 * (time.perf_counter() - t0)
            cd = hip.webp_code(data, r * W, *tb)
            assert np.array_equal(cd[1].cpu().numpy(), tb[2][:, 1:])
            return hist, tb, host_ms, cd

        blobs = video_out.encode_webp_frames(frames)
        host = frames.cpu().numpy()
        k = min(a.pil_frames, n)
        rec = {"input": kind, "frames": n, "size": [H, W], "strip_rows": rows, "box": torch.cuda.get_device_name(0), "bytes_raw": int(frames.numel()),
               "webp_bytes": sum(len(b) for b in blobs), "png_stream_bytes": sum(len(b) for b in video_out.encode_png_frames(frames)),
               "pil_frames": k, "webp_bytes_pil_frames": sum(len(b) for b in blobs[:k]),
               "pil_webp_method0_bytes": pil_webp_bytes(host[:k], 0), "pil_webp_method4_bytes": pil_webp_bytes(host[:k], 4)}
        if kind in ("vae", "pose"):
            sweep = []
            for r in a.sweep:
                r = min(r, H)
                h_r, tb_r, host_r, c_r = stages(r)
                reps = max(3, a.reps // 4)
                sweep.append({"strip_rows": r, "workgroups": int(tb_r[2][:, 1:].size),
                              "histogram_ms": round(timed(lambda: hip.webp_histogram(data, r * W, out=h_r), reps), 3),
                              "code_ms": round(timed(lambda: hip.webp_code(data, r * W, *tb_r, out=c_r), reps), 3), "host_tables_ms": round(host_r, 1),
                              "payload_bytes": int(((tb_r[2].sum(1) + 7) // 8).sum())})
            rec["strip_rows_sweep"] = sweep
        if kind == "vae":
            hist, tb, host_ms, cd = stages(rows)
            pk = hip.webp_pack(cd[0], tb[2])
            rec.update({"predict_ms_per_frame": round(timed(lambda: hip.webp_predict(frames, out=po), a.reps) / n, 4),
                        "histogram_ms_per_frame": round(timed(lambda: hip.webp_histogram(data, rows * W, out=hist), a.reps) / n, 4),
                        "code_ms_per_frame": round(timed(lambda: hip.webp_code(data, rows * W, *tb, out=cd), a.reps) / n, 4),
                        "pack_ms_per_frame": round(timed(lambda: hip.webp_pack(cd[0], tb[2], out=pk[0]), a.reps) / n, 4),
                        "copy_ms_per_frame": round(timed(lambda: pk[0].cpu(), a.reps) / n, 4), "host_tables_ms_per_frame": round(host_ms / n, 3)})
            # end to end, alternating; host frames in (what save_videos_grid is handed), files out
            clip = frames.cpu()[None]
            ours, theirs = os.path.join(tmp, "clip.webp"), os.path.join(tmp, "pil.webp")
            acc = {"pil": [], "device": []}
            video_out.save_videos_grid(clip, ours, fps=25)                                 # warm
            for _ in range(a.pairs):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                pil = [Image.fromarray(f) for f in clip[0].numpy()]
                pil[0].save(theirs, format="WEBP", lossless=True, method=0, save_all=True, append_images=pil[1:], duration=40, loop=0)
                acc["pil"].append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                video_out.save_videos_grid(clip, ours, fps=25)
                torch.cuda.synchronize()
                acc["device"].append(time.perf_counter() - t0)
            for name in acc:
                rec[f"save_{name}_ms"] = [round(1e3 * t, 1) for t in acc[name]]
                rec[f"save_{name}_ms_median"] = round(1e3 * sorted(acc[name])[len(acc[name]) // 2], 1)
            rec["file_bytes_webp"] = os.path.getsize(ours)
            rec["file_bytes_pil_webp_method0"] = os.path.getsize(theirs)
            os.remove(ours)
            os.remove(theirs)
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
    os.rmdir(tmp)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
