#!/usr/bin/env python3
"""Motion-JPEG encoder timings on one MI355X, one JSON line per clip length (24 and 96 frames of 512 x 512, quality 90, 4:2:0):

  * device time of the three stages by HIP events: dct_quant, entropy, scan + compact (frames of a VAE decode with random-init weights);
    the DCT stage also as bytes moved (frame read + int16 coefficients written) over its time, against the HBM peak;
  * bytes out;
  * end to end on the same box, alternating: latents -> JPEG bytes on the host (AutoencoderKL.decode_video_jpeg) against
    latents -> uint8 frames on the host (decode_video_uint8(...).cpu(), the path before the encoder existed); host clock around work that
    ends in a synchronising copy.

    python tools/bench_mjpeg.py [--reps 20] [--pairs 5] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK_TBS = 8.0          # MI355X HBM3E peak


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


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--pairs", type=int, default=5)
    p.add_argument("--quality", type=int, default=90)
    p.add_argument("--out", type=str, default=None)
    a = p.parse_args()
    from mmgt_amd import hip, video_out
    from mmgt_amd.synthetic import hash_uniform, synth_state_dict
    from mmgt_amd.vae import AutoencoderKL, vae_decoder_spec
    dev = torch.device("cuda:0")
    vae = AutoencoderKL(device=dev, dtype=torch.bfloat16)
    vae.load_state_dict(synth_state_dict(vae_decoder_spec(), prefix="vae.", device=dev))
    lines = []
    for n in (24, 96):
        lat = hash_uniform("bench.mjpeg.lat", (1, 4, n, 64, 64), 1.7).to(dev)
        frames = vae.decode_video_uint8(lat)[0].contiguous()                              # (n, 512, 512, 3) on the device
        H, W = frames.shape[1:3]
        rows = hip.jpeg_geometry(H, W, "4:2:0")[0]
        coef = hip.jpeg_dct_quant(frames, a.quality)
        out = hip.jpeg_entropy(coef, H, W)
        data, off = hip.jpeg_compact(out[0], out[1], rows)
        offsets = off.to(dev)
        t_dct = timed(lambda: hip.jpeg_dct_quant(frames, a.quality), a.reps)
        t_ent = timed(lambda: hip.jpeg_entropy(coef, H, W, out=out), a.reps)

        def compact():
            lib, st = hip.lib(), torch.cuda.current_stream().cuda_stream
            lib.mmgt_jpeg_scan(out[1].data_ptr(), offsets.data_ptr(), n * rows, st)
            lib.mmgt_jpeg_compact(out[0].data_ptr(), out[0].shape[1], out[1].data_ptr(), offsets.data_ptr(), data.data_ptr(), data.numel(), n * rows,
                                  rows, st)
        t_cmp = timed(compact, a.reps)
        dct_bytes = frames.numel() + coef.numel() * 2
        rec = {"frames": n, "size": [H, W], "quality": a.quality, "subsampling": "4:2:0", "box": torch.cuda.get_device_name(0),
               "dct_quant_us": round(1e3 * t_dct, 1), "entropy_us": round(1e3 * t_ent, 1), "scan_compact_us": round(1e3 * t_cmp, 1),
               "dct_quant_us_per_frame": round(1e3 * t_dct / n, 2), "dct_quant_GBs": round(dct_bytes / t_dct / 1e6, 1),
               "dct_quant_share_of_hbm_peak": round(dct_bytes / t_dct / 1e6 / (1e3 * HBM_PEAK_TBS), 3),
               "bytes_out": int(data.numel()) + n * len(video_out.jfif_headers(W, H, a.quality)), "bytes_raw": int(frames.numel()),
               "segment_scratch_bytes": int(out[0].numel())}
        # end to end, alternating the two paths
        jpeg_s, u8_s = [], []
        for f in (lambda: vae.decode_video_jpeg(lat, a.quality), lambda: vae.decode_video_uint8(lat).cpu()):
            f()                                                                           # warm both
        for _ in range(a.pairs):
            for f, acc in ((lambda: vae.decode_video_jpeg(lat, a.quality), jpeg_s), (lambda: vae.decode_video_uint8(lat).cpu(), u8_s)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()
                torch.cuda.synchronize()
                acc.append(time.perf_counter() - t0)
        rec.update(latents_to_jpeg_host_ms=[round(1e3 * t, 2) for t in jpeg_s], latents_to_uint8_host_ms=[round(1e3 * t, 2) for t in u8_s],
                   latents_to_jpeg_host_ms_median=round(1e3 * sorted(jpeg_s)[len(jpeg_s) // 2], 2),
                   latents_to_uint8_host_ms_median=round(1e3 * sorted(u8_s)[len(u8_s) // 2], 2))
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
