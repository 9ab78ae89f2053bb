#!/usr/bin/env python3
"""Device lossy WebP (VP8 key frame) encoder on one MI355X, one JSON line per input kind (24 frames of 512 x 512; the clips of tools/bench_webp.py:
`vae`, `smooth`, `mask`, `pose`):

  * bytes and PSNR (PIL's decode against the source, over the first --pil-frames frames) at qualities 10 .. 100, beside the lossless .webp
    payloads (encode_webp_frames), the .avi frames at quality 90 (encode_jpeg_frames) and PIL's own lossy writer at methods 0 and 4, quality 75;
  * on `vae`: device time of the stages by HIP events, as ms per frame: convert, analyse (ONE workgroup per frame walks the anti-diagonals), code
    (one lane per partition), pack (with the read-back of the counts), the copy of the finished bytes to the host;
  * on `vae`: coding time and payload bytes for 1 / 2 / 4 / 8 token partitions;
  * on `vae`: analyse time of 1 frame against all frames, which shows what one workgroup per frame leaves idle;
  * on `vae`: end to end on the same box, alternating: save_videos_grid(frames, "x.webp", webp_quality=75) against PIL's animated
    Image.save(format="WEBP", quality=75, method=0, save_all=True) of the same host frames; host clock, host uint8 frames in, file out.

    python tools/bench_vp8.py [--reps 10] [--pairs 3] [--out profiles/vp8/bench_vp8.jsonl]"""
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_webp import mask_clip, pose_clip, smooth_clip, timed  # noqa: E402


def psnr(a, b):
    mse = ((a.astype(np.float64) - b.astype(np.float64)) ** 2).mean()
    return 99.0 if mse == 0 else float(10 * np.log10(255 ** 2 / mse))


def decode(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def still(payload):
    import struct
    body = b"WEBP" + b"VP8 " + struct.pack("<I", len(payload)) + payload + (b"\0" if len(payload) & 1 else b"")
    return b"RIFF" + struct.pack("<I", len(body)) + body


def pil_lossy(frames, method, quality):
    from PIL import Image
    total, ps = 0, []
    for f in frames:
        buf = io.BytesIO()
        Image.fromarray(f).save(buf, format="WEBP", quality=quality, method=method)
        total += buf.tell() - 20
        ps.append(psnr(decode(buf.getvalue()), f))
    return total, round(float(np.mean(ps)), 2)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--pairs", type=int, default=3)
    p.add_argument("--frames", type=int, default=24)
    p.add_argument("--pil-frames", type=int, default=4)
    p.add_argument("--qualities", type=int, nargs="+", default=[10, 30, 50, 75, 90, 100])
    p.add_argument("--out", type=str, default=os.path.join("profiles", "vp8", "bench_vp8.jsonl"))
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
    tmp = tempfile.mkdtemp(prefix="bench_vp8_")
    for kind, frames in clips.items():
        H, W = frames.shape[1:3]
        host = frames.cpu().numpy()
        k = min(a.pil_frames, n)
        rec = {"input": kind, "frames": n, "size": [H, W], "box": torch.cuda.get_device_name(0), "bytes_raw": int(frames.numel()),
               "webp_lossless_bytes": sum(len(b) for b in video_out.encode_webp_frames(frames)),
               "avi_q90_bytes": sum(len(b) for b in video_out.encode_jpeg_frames(frames, 90)), "pil_frames": k, "by_quality": []}
        for quality in a.qualities:
            blobs = video_out.encode_vp8_frames(frames, quality)
            rec["by_quality"].append({"quality": quality, "q": hip.vp8_quantiser(quality)[0], "filter_level": hip.vp8_quantiser(quality)[1],
                                      "bytes": sum(len(b) for b in blobs), "bytes_pil_frames": sum(len(b) for b in blobs[:k]),
                                      "psnr": round(float(np.mean([psnr(decode(still(blobs[f])), host[f]) for f in range(k)])), 2)})
        for method in (0, 4):
            rec[f"pil_lossy_q75_method{method}_bytes"], rec[f"pil_lossy_q75_method{method}_psnr"] = pil_lossy(host[:k], method, 75)
        if kind == "vae":
            q, level = hip.vp8_quantiser(75)
            parts = video_out.vp8_default_partitions(H)
            planes = hip.vp8_convert(frames)
            an = hip.vp8_analyse(planes, H, W, q)
            cd = hip.vp8_code(an[1], an[3], an[2], an[4], H, W, q, parts, level)
            pk = hip.vp8_pack(*cd, H, W, parts)
            rec.update({"quality": 75, "partitions": parts,
                        "convert_ms_per_frame": round(timed(lambda: hip.vp8_convert(frames, out=planes), a.reps) / n, 4),
                        "analyse_ms_per_frame": round(timed(lambda: hip.vp8_analyse(planes, H, W, q, out=an), a.reps) / n, 4),
                        "code_ms_per_frame": round(timed(lambda: hip.vp8_code(an[1], an[3], an[2], an[4], H, W, q, parts, level, out=cd), a.reps) / n, 4),
                        "pack_ms_per_frame": round(timed(lambda: hip.vp8_pack(*cd, H, W, parts, out=pk[0]), a.reps) / n, 4),
                        "copy_ms_per_frame": round(timed(lambda: pk[0].cpu(), a.reps) / n, 4)})
            one = tuple(t[:1] for t in planes)
            an1 = hip.vp8_analyse(one, H, W, q)
            rec["analyse_ms_one_frame"] = round(timed(lambda: hip.vp8_analyse(one, H, W, q, out=an1), a.reps), 3)
            rec["analyse_ms_all_frames"] = round(rec["analyse_ms_per_frame"] * n, 3)
            sweep = []
            for P in (1, 2, 4, 8):
                c = hip.vp8_code(an[1], an[3], an[2], an[4], H, W, q, P, level)
                sweep.append({"partitions": P, "code_ms": round(timed(lambda: hip.vp8_code(an[1], an[3], an[2], an[4], H, W, q, P, level, out=c), a.reps), 3),
                              "payload_bytes": int(c[1].sum().item()) + n * (10 + 3 * (P - 1))})
            rec["partition_sweep"] = sweep
            clip = frames.cpu()[None]
            ours, theirs = os.path.join(tmp, "clip.webp"), os.path.join(tmp, "pil.webp")
            acc = {"pil": [], "device": []}
            video_out.save_videos_grid(clip, ours, fps=25, webp_quality=75)                # warm
            for _ in range(a.pairs):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                pil = [Image.fromarray(f) for f in clip[0].numpy()]
                pil[0].save(theirs, format="WEBP", quality=75, method=0, save_all=True, append_images=pil[1:], duration=40, loop=0)
                acc["pil"].append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                video_out.save_videos_grid(clip, ours, fps=25, webp_quality=75)
                torch.cuda.synchronize()
                acc["device"].append(time.perf_counter() - t0)
            for name in acc:
                rec[f"save_{name}_ms"] = [round(1e3 * t, 1) for t in acc[name]]
                rec[f"save_{name}_ms_median"] = round(1e3 * sorted(acc[name])[len(acc[name]) // 2], 1)
            rec["file_bytes_webp_q75"] = os.path.getsize(ours)
            rec["file_bytes_pil_q75_method0"] = os.path.getsize(theirs)
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
