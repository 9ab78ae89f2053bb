#!/usr/bin/env python3
"""WavLM-Large timings on one MI355X (HIP events), one JSON line: slice_features for 1 / 4 / 16 slices of 3.2 s (bf16 product mode,
hash-seeded Large weights), and mmgt_relpos_attention at (B x 16 heads, T = 159) and T = 1500 against the same attention composed from
existing pieces (mmgt_gemm scores, a torch add of the materialised gated bias, mmgt_softmax_rows, mmgt_gemm for P.V; tool-only).

    python tools/bench_wavlm.py [--reps 20]"""
import argparse
import json
import os
import sys

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


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=20)
    a = p.parse_args()
    from mmgt_amd import hip
    from mmgt_amd.synthetic import hash_uniform, synth_state_dict
    from mmgt_amd.wavlm import WavLM, WavLMConfig, relative_position_buckets, wavlm_spec
    dev, dt = torch.device("cuda:0"), torch.bfloat16
    res = {"box": torch.cuda.get_device_name(0)}
    H, C = 16, 1024
    for B, T in ((1, 159), (4, 159), (1, 1500)):
        qkv = hash_uniform(f"bw.qkv{T}", (B * T, 3 * C), 1.0, dev).to(dt)
        x = hash_uniform(f"bw.x{T}", (B * T, C), 1.0, dev).to(dt)
        gw, gb = hash_uniform("bw.gw", (8, 64), 0.3, dev), hash_uniform("bw.gb", (8,), 0.5, dev)
        ga = 1.0 + hash_uniform("bw.ga", (H,), 0.5, dev)
        tab = hash_uniform("bw.emb", (320, H), 2.0, dev)[relative_position_buckets(T).to(dev)].t().contiguous()
        out = torch.empty((B * T, C), device=dev, dtype=dt)
        st3, st1 = (T * 3 * C, 3 * C), (T * C, C)
        f = lambda: hip.relpos_attention(qkv, qkv[:, C:], qkv[:, 2 * C:], out, x, gw, gb, ga, tab, batch=B, heads=H, T=T, scale=0.125,
                                         q_str=st3, k_str=st3, v_str=st3, o_str=st1, x_str=st1)
        res[f"relpos_attn_B{B}_T{T}_us"] = round(1000 * timed(f, a.reps), 1)
        # composed from existing pieces: per (b, h) a scores GEMM, the gated bias added by torch, softmax rows, a P.V GEMM
        idx = (torch.arange(T, device=dev)[None, :] - torch.arange(T, device=dev)[:, None] + T - 1)
        bias = tab[:, idx]                                                            # (H, T, T) fp32
        gate = torch.rand((B, H, T, 1), device=dev) + 1.0
        gb_full = (gate * bias[None]).to(dt)                                          # materialised (B, H, T, T)
        Tp = (T + 63) // 64 * 64
        q = qkv[:, :C].reshape(B, T, H, 64).permute(0, 2, 1, 3).contiguous()
        k = qkv[:, C:2 * C].reshape(B, T, H, 64).permute(0, 2, 1, 3).contiguous()
        vt = torch.zeros((B, H, 64, Tp), device=dev, dtype=dt)
        vt[..., :T] = qkv[:, 2 * C:].reshape(B, T, H, 64).permute(0, 2, 3, 1)
        s = torch.empty((T, Tp), device=dev, dtype=dt)[:, :T]
        pr = torch.zeros((T, Tp), device=dev, dtype=dt)
        o2 = torch.empty((T, 64), device=dev, dtype=dt)

        def composed():
            for b in range(B):
                for h in range(H):
                    hip.gemm(q[b, h], k[b, h], out=s, alpha=0.125)
                    s.add_(gb_full[b, h])
                    hip.softmax_rows(s, out=pr[:, :T])
                    hip.gemm(pr, vt[b, h], out=o2)
        res[f"composed_B{B}_T{T}_us"] = round(1000 * timed(composed, max(2, a.reps // 4), warm=1), 1)
    m = WavLM(WavLMConfig(), device=dev, dtype=dt)
    m.load_state_dict(synth_state_dict(wavlm_spec(), prefix="wavlm.", device=dev))
    for n in (1, 4, 16):
        waves = hash_uniform(f"bw.wave{n}", (n, 51200), 0.5, dev)
        res[f"slice_features_{n}_ms"] = round(timed(lambda: m.slice_features(waves), max(2, a.reps // 4), warm=1), 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
