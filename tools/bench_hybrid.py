#!/usr/bin/env python3
"""Step time of a hybrid-conditioned model on the GPU, beside the crossattn model in the same process:

  hybrid     full-width UNet with in_channels = 8, key 'hybrid': x [1, 4, 16, 40, 64] + one c_concat [1, 4, 16, 40, 64], 77 tokens;
  crossattn  full-width UNet with in_channels = 4, key 'crossattn': x [1, 4, 16, 40, 64], 77 tokens.

Both through `DenoiseModel.apply_model` (one UNet forward, replayed as a hipGraph), alternating, warm-up first, median over the
repetitions; one JSON line each.  The expectation is equal step times: the first conv already pads K to 8 channels per tap.

    python tools/bench_hybrid.py [--reps N] [--warmup W]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
UNET = "lvdm.modules.networks.openaimodel3d.UNetModel"


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n             # ms per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=5)
    a = ap.parse_args()
    from helpers import FULL, inp
    from moca_video_amd import DenoiseModel
    from moca_video_amd.weightgen import gen_state_dict
    torch.cuda.set_device(0)
    shp = (16, 40, 64)
    x = inp("bench_hybrid.x", (1, 4) + shp).cuda()
    cc = inp("bench_hybrid.cc", (1, 4) + shp).cuda()
    ctx = inp("bench_hybrid.ctx", (1, 77, 1024)).cuda()
    t = torch.tensor([500]).cuda()
    calls = {}
    for key, cin in (("hybrid", 8), ("crossattn", 4)):
        m = DenoiseModel({"target": UNET, "params": dict(FULL, in_channels=cin)}, conditioning_key=key)
        unet = m.model.diffusion_model
        unet.load_state_dict(gen_state_dict({k: v.shape for k, v in unet.state_dict().items()}, 11), strict=True)
        m = m.cuda()
        cond = {"c_crossattn": [ctx]}
        if key == "hybrid":
            cond["c_concat"] = [cc]
        calls[key] = (lambda m=m, cond=cond: m.apply_model(x, t, cond))
    for f in calls.values():
        timed(f, max(a.warmup, 3))            # eager pass, capture pass, replays
    times = {k: [] for k in calls}
    for _ in range(a.reps):
        for k, f in calls.items():
            times[k].append(timed(f, a.inner))
    for k, cin in (("hybrid", 8), ("crossattn", 4)):
        print(json.dumps({"bench": "unet_step", "conditioning_key": k, "in_channels": cin, "latents": [1, cin, 16, 40, 64], "context_tokens": 77,
                          "device": torch.cuda.get_device_name(0), "reps": a.reps, "inner": a.inner, "warmup": max(a.warmup, 3),
                          "median_ms": round(statistics.median(times[k]), 4), "min_ms": round(min(times[k]), 4),
                          "max_ms": round(max(times[k]), 4)}), flush=True)


if __name__ == "__main__":
    main()
