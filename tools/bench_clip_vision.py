#!/usr/bin/env python3
"""Image embedder timings on the GPU (first measurements; no target exists): HIP-event ms per image of FrozenOpenCLIPImageEmbedderV2
at full ViT-H/14 size on 320 x 512 images, B = 1 and 2 (preprocess + patch GEMM + 32 blocks, eager launches on the current stream), and
the isolated moca_attention_d80_f16 at N = 257, heads = 16 in TFLOP/s (4 N^2 80 heads B FLOP per launch).

    python tools/bench_clip_vision.py [--reps N]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed_ms(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from moca_video_amd import ops
    from moca_video_amd.clip_vision import FrozenOpenCLIPImageEmbedderV2
    from moca_video_amd.weightgen import init_random_
    assert torch.cuda.is_available(), "needs the GPU"
    res = {}
    m = init_random_(FrozenOpenCLIPImageEmbedderV2().cuda(), 0)
    g = torch.Generator(device="cuda").manual_seed(0)
    for B in (1, 2):
        img = torch.rand(B, 3, 320, 512, device="cuda", generator=g) * 2 - 1
        fn = lambda: m(img)
        timed_ms(fn, 3)                                   # warm-up (packs the weights on the first call)
        t = [timed_ms(fn, 10) for _ in range(args.reps)]
        res[f"v2_ms_per_image_b{B}"] = round(statistics.median(t) / B, 3)
        res[f"v2_ms_per_call_b{B}_min"] = round(min(t), 3)
    del m
    torch.cuda.empty_cache()
    for B in (1, 8):
        N, H, C = 257, 16, 1280
        qkv = torch.randn(B * N, 3 * C, device="cuda", generator=g).half()
        out = torch.empty(B * N, C, dtype=torch.float16, device="cuda")
        fn = lambda: ops.attention_d80(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], out, B=B, heads=H, N=N, ldq=3 * C, ldk=3 * C,
                                       ldv=3 * C, ldo=C, scale=80 ** -0.5)
        timed_ms(fn, 20)
        t = statistics.median(timed_ms(fn, 200) for _ in range(args.reps))
        res[f"attn_d80_b{B}_us"] = round(t * 1e3, 2)
        res[f"attn_d80_b{B}_tflops"] = round(4 * N * N * 80 * H * B / (t * 1e-3) / 1e12, 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
