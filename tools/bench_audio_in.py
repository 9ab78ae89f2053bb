#!/usr/bin/env python3
"""Audio input timings on one MI355X, one JSON line per input; the files are seeded noise-plus-tones written by tests/audio_ref.py:

  * s16_stereo_44k1_60s    60 s of 44.1-kHz stereo 16-bit PCM  (160 / 441, 59 571 taps, 373 per output)
  * f32_mono_48k_60s       60 s of 48-kHz mono 32-bit float    (1 / 3, 407 taps, all of them per output)
  * s16_stereo_44k1_3s2    3.2 s of the first: one SMGA slice, the short clip a user of scripts/audio2vid.py starts with

Per input: device time by HIP events of the decode launch and of the resample launch on operands that are already on the device, the bytes each
must move (read + written once; the tap table and the re-read of staged inputs stay in cache and are not counted) as a rate and as a share of
the 8 TB/s HBM peak; and end to end on the same box, alternating, host clock around work that ends in a synchronise: file bytes in memory ->
mono fp32 16-kHz tensor on the device, through read_audio_device and through the host route -- numpy decode and down-mix,
scipy.signal.resample_poly with the SAME taps, upload.  The line holds the largest difference between the two routes' results.

    python tools/bench_audio_in.py [--reps 20] [--pairs 7] [--out FILE]     (default: rewrites profiles/audio_in/bench_audio_in.jsonl)"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12


def signal(seconds, rate, channels):
    rng = np.random.default_rng(20261021)
    t = np.arange(int(seconds * rate)) / rate
    x = 0.3 * np.sin(2 * np.pi * 220 * t) + 0.2 * np.sin(2 * np.pi * 3100 * t) + 0.1 * rng.uniform(-1, 1, t.shape)
    return np.stack([x * (1.0 - 0.1 * c) for c in range(channels)], axis=1)


def timed(fn, reps, warm=3):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    total = 0.0
    for rep in range(warm + reps):
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        total += e0.elapsed_time(e1) if rep >= warm else 0.0
    return total / reps


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--pairs", type=int, default=7)
    p.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "audio_in", "bench_audio_in.jsonl"))
    a = p.parse_args()
    from scipy.signal import resample_poly
    from mmgt_amd import audio_in as A
    from mmgt_amd import hip
    from tests import audio_ref as R
    assert torch.cuda.is_available(), "bench_audio_in needs an MI355X: nothing here is a CPU timing"
    dev = torch.device("cuda:0")
    lines = []
    for name, fmt, channels, rate, seconds in (("s16_stereo_44k1_60s", R.S16, 2, 44100, 60.0), ("f32_mono_48k_60s", R.F32, 1, 48000, 60.0),
                                               ("s16_stereo_44k1_3s2", R.S16, 2, 44100, 3.2)):
        wav = R.wav_bytes(R.encode_frames(signal(seconds, rate, channels), fmt), fmt, channels, rate)
        info = A.parse_wav(wav)
        n = info.data_bytes // info.block_align
        up, down, half, h = A.resample_plan(rate)
        raw = torch.frombuffer(bytearray(wav[info.data_offset:info.data_offset + info.data_bytes]), dtype=torch.uint8).to(dev)
        mono = hip.audio_decode_mono(raw, n, channels, fmt)
        y = A.resample_device(mono, rate)
        table = A.plan_cache()[(rate, 16000, str(mono.device))][3]
        t_dec = timed(lambda: hip.audio_decode_mono(raw, n, channels, fmt, out=mono), a.reps)
        t_res = timed(lambda: hip.audio_resample(mono, table, up, down, half, out=y), a.reps)
        b_dec, b_res = info.data_bytes + 4 * n, 4 * n + 4 * y.numel()

        def host():
            i = A.parse_wav(wav)
            v = np.frombuffer(wav, dtype="<i2" if fmt == R.S16 else "<f4", count=i.data_bytes // (2 if fmt == R.S16 else 4), offset=i.data_offset)
            m = v.reshape(-1, channels).astype(np.float32).mean(1) / (32768.0 if fmt == R.S16 else 1.0)
            return torch.from_numpy(resample_poly(m, up, down, window=h / up).astype(np.float32)).to(dev)

        routes = {"device": lambda: A.read_audio_device(wav, device=dev), "host_scipy": host}
        first = {k: f() for k, f in routes.items()}                                             # also warms both routes
        times = {k: [] for k in routes}
        for _ in range(a.pairs):
            for k, f in routes.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()
                torch.cuda.synchronize()
                times[k].append(time.perf_counter() - t0)
        med = lambda v: sorted(v)[len(v) // 2]
        rec = {"input": name, "fmt": R.NAMES[fmt], "channels": channels, "rate": rate, "seconds": seconds, "frames": n, "file_bytes": len(wav),
               "up": up, "down": down, "taps": 2 * half + 1, "taps_per_output": 2 * half // up + 1, "samples_16k": int(y.numel()),
               "box": torch.cuda.get_device_name(0), "decode_us": round(1e3 * t_dec, 2), "resample_us": round(1e3 * t_res, 2),
               "decode_bytes": b_dec, "resample_bytes": b_res, "decode_GBps": round(b_dec / (1e-3 * t_dec) / 1e9, 1),
               "resample_GBps": round(b_res / (1e-3 * t_res) / 1e9, 1), "decode_share_of_hbm_peak": round(b_dec / (1e-3 * t_dec) / HBM_PEAK, 4),
               "resample_share_of_hbm_peak": round(b_res / (1e-3 * t_res) / HBM_PEAK, 4),
               "resample_gfma_per_s": round(y.numel() * (2 * half // up + 1) / (1e-3 * t_res) / 1e9, 1),
               "max_abs_device_minus_host": float((first["device"] - first["host_scipy"]).abs().max())}
        for k, v in times.items():
            rec[k + "_ms"] = [round(1e3 * t, 2) for t in v]
            rec[k + "_ms_median"] = round(1e3 * med(v), 2)
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
