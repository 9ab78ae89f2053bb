#!/usr/bin/env python3
"""Device PNG encoder timings on one MI355X, one JSON line per clip length (24 frames of 512 x 512 out of a VAE decode with random-init weights):

  * device time of the stages by HIP events, as ms per frame: filter, histogram, deflate (with the upload of its tables), pack, and the copy of the
    finished bytes to the host; the host's code building (deflate_code_lengths + deflate_block_header for every strip) in ms per frame;
  * histogram + host tables + deflate time and stream size for several strip_rows (the choice of video_out.PNG_STRIP_ROWS), strip_rows = H being
    one deflate block per frame;
  * end to end on the same box, alternating: save_videos_grid(frames, "x.apng") against PIL's Image.save(format="PNG") per frame of the same
    host frames (what a caller without this writer does after downloading them); host clock, host uint8 frames in, encoded bytes out;
  * file sizes: the .apng, PIL's PNG files together, and zlib's Z_RLE and default strategies on the device's filtered bytes.

    python tools/bench_png.py [--reps 20] [--pairs 3] [--out profiles/png/bench_png.jsonl]"""
import argparse
import io
import json
import os
import sys
import tempfile
import time
import zlib

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


def tables(hist, hip, video_out):
    k, strips = hist.shape[:2]
    codes = np.empty((k, strips, 286), np.uint32)
    heads, hbits = np.zeros((k, strips, hip.PNG_HEADER_BYTES), np.uint8), np.empty((k, strips), np.int32)
    want = np.empty((k, strips), np.int64)
    for f in range(k):
        for s in range(strips):
            codes[f, s], head, hbits[f, s], want[f, s] = video_out.png_strip_tables(hist[f, s], s == strips - 1)
            heads[f, s, :len(head)] = np.frombuffer(head, np.uint8)
    return codes, heads, hbits, want


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--pairs", type=int, default=3)
    p.add_argument("--frames", type=int, nargs="+", default=[24])
    p.add_argument("--sweep", type=int, nargs="+", default=[4, 8, 16, 32, 64, 512])
    p.add_argument("--out", type=str, default=os.path.join("profiles", "png", "bench_png.jsonl"))
    a = p.parse_args()
    from PIL import Image
    from mmgt_amd import hip, video_out
    from mmgt_amd.synthetic import hash_uniform, synth_state_dict
    from mmgt_amd.vae import AutoencoderKL, vae_decoder_spec
    dev = torch.device("cuda:0")
    vae = AutoencoderKL(device=dev, dtype=torch.bfloat16)
    vae.load_state_dict(synth_state_dict(vae_decoder_spec(), prefix="vae.", device=dev))
    lines = []
    tmp = tempfile.mkdtemp(prefix="bench_png_")
    for n in a.frames:
        lat = hash_uniform("bench.gif.lat", (1, 4, n, 64, 64), 1.7).to(dev)
        frames = vae.decode_video_uint8(lat)[0].contiguous()                              # (n, 512, 512, 3) on the device
        H, W = frames.shape[1:3]
        L = 1 + 3 * W
        rows = min(video_out.PNG_STRIP_ROWS, H)
        fo = hip.png_filter(frames)
        data = fo[0].view(n, H * L)

        def stages(r):
            hist = hip.png_histogram(data, r * L)
            h = hist.cpu().numpy().view(np.uint32).astype(np.int64)
            t0 = time.perf_counter()
            tb = tables(h, hip, video_out)
            host_ms = 1e3 * (time.perf_counter() - t0)
            dfl = hip.png_deflate(data, r * L, *tb)
            assert np.array_equal(dfl[1].cpu().numpy(), tb[3])
            return hist, tb, host_ms, dfl

        hist, tb, host_ms, dfl = stages(rows)
        pk = hip.png_pack(dfl[0], tb[3])
        t_filter = timed(lambda: hip.png_filter(frames, out=fo), a.reps)
        t_hist = timed(lambda: hip.png_histogram(data, rows * L, out=hist), a.reps)
        t_dfl = timed(lambda: hip.png_deflate(data, rows * L, *tb, out=dfl), a.reps)
        t_pack = timed(lambda: hip.png_pack(dfl[0], tb[3], out=pk[0]), a.reps)
        t_copy = timed(lambda: pk[0].cpu(), a.reps)
        sweep = []
        for r in a.sweep:
            r = min(r, H)
            h_r, tb_r, host_r, d_r = stages(r)
            reps = max(3, a.reps // 4)
            sweep.append({"strip_rows": r, "workgroups": int(tb_r[3].size), "histogram_ms": round(timed(lambda: hip.png_histogram(data, r * L, out=h_r), reps), 3),
                          "deflate_ms": round(timed(lambda: hip.png_deflate(data, r * L, *tb_r, out=d_r), reps), 3), "host_tables_ms": round(host_r, 1),
                          "stream_bytes": int(((tb_r[3].sum(1) + 7) // 8).sum())})
        filt_h = fo[0].cpu().numpy()
        z_rle, z_def = 0, 0
        for f in range(n):
            for strategy in (zlib.Z_RLE, zlib.Z_DEFAULT_STRATEGY):
                c = zlib.compressobj(6, zlib.DEFLATED, -15, 9, strategy)
                size = len(c.compress(filt_h[f].tobytes()) + c.flush())
                if strategy == zlib.Z_RLE:
                    z_rle += size
                else:
                    z_def += size
        rec = {"frames": n, "size": [H, W], "strip_rows": rows, "box": torch.cuda.get_device_name(0),
               "filter_ms_per_frame": round(t_filter / n, 4), "histogram_ms_per_frame": round(t_hist / n, 4),
               "deflate_ms_per_frame": round(t_dfl / n, 4), "pack_ms_per_frame": round(t_pack / n, 4), "copy_ms_per_frame": round(t_copy / n, 4),
               "host_tables_ms_per_frame": round(host_ms / n, 3), "strip_rows_sweep": sweep, "bytes_raw": int(frames.numel()),
               "stream_bytes": int(pk[1][-1]), "zlib_rle_bytes_same_filtered_rows": z_rle, "zlib_default_bytes_same_filtered_rows": z_def}
        # end to end, alternating; host frames in (what save_videos_grid is handed), files out
        host = frames.cpu()[None]
        apng = os.path.join(tmp, f"clip_{n}.apng")
        acc = {"pil": [], "device": []}
        pil_bytes = 0
        video_out.save_videos_grid(host, apng, fps=25)                                     # warm
        for _ in range(a.pairs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pil_bytes = 0
            for f in host[0].numpy():
                buf = io.BytesIO()
                Image.fromarray(f).save(buf, format="PNG")
                pil_bytes += buf.tell()
            acc["pil"].append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            video_out.save_videos_grid(host, apng, fps=25)
            torch.cuda.synchronize()
            acc["device"].append(time.perf_counter() - t0)
        for k in acc:
            rec[f"save_{k}_ms"] = [round(1e3 * t, 1) for t in acc[k]]
            rec[f"save_{k}_ms_median"] = round(1e3 * sorted(acc[k])[len(acc[k]) // 2], 1)
        rec["file_bytes_apng"] = os.path.getsize(apng)
        rec["file_bytes_pil_pngs"] = pil_bytes
        os.remove(apng)
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
    os.rmdir(tmp)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
