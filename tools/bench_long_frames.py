#!/usr/bin/env python3
"""Cost of clips longer than 16 frames on the GPU, HIP events, one JSON line per figure:

  kernel    moca_temporal_attention_long_f16 at (B, T, HW, heads) = (1, 32, 2560, 5) and (1, 24, 2560, 5) beside the 16-frame kernel
            moca_temporal_attention_f16 at (1, 16, 2560, 5) in the SAME process, alternating: the three read q, k and v once and write
            out once (4 * T * HW * heads * 64 * 2 bytes), so bytes per second is the yardstick between them.  A sample is the time of
            `--inner` back-to-back launches between two events, divided by their number.
  forward   the B = 2 shared-prefix forward (the two branches of classifier-free guidance on one x) of the full-width UNet at
            [1,4,24,40,64] and [1,4,32,40,64], 77 tokens: eager pass, capture and replays as warm-up, then one sample per replay.

Every figure is the median of `--reps` (>= 20) samples after warm-up.  Each step runs in a child process of its own under its own time
limit (`timeout`); the first step that fails ends the run.

    python tools/bench_long_frames.py [--reps N] [--inner K] [--only kernel|forward24|forward32]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
STEPS = {"kernel": 240, "forward24": 420, "forward32": 420}       # seconds (the forwards pack the full-width weights first)


def _summary(ms):
    return {"median_ms": round(statistics.median(ms), 5), "min_ms": round(min(ms), 5), "max_ms": round(max(ms), 5)}


def kernel(reps, inner):
    import torch
    from helpers import inp
    from moca_video_amd import ops
    torch.cuda.set_device(0)
    HW, heads = 2560, 5
    C = heads * 64
    cases = {}
    for T in (16, 24, 32):
        qkv = inp(f"bench_lf.qkv{T}", (T * HW, 3 * C)).half().cuda()
        out = torch.empty(T * HW, C, dtype=torch.float16, device="cuda")
        kw = dict(B=1, T=T, HW=HW, heads=heads, ld_qkv=3 * C, ldo=C, scale=0.125)
        fn = ops.temporal_attention if T == 16 else ops.temporal_attention_long
        cases[T] = (lambda fn=fn, qkv=qkv, out=out, kw=kw: fn(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], out, **kw))

    def sample(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            call()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / inner
    for call in cases.values():                      # warm-up: code objects, clocks
        for _ in range(3):
            sample(call)
    times = {T: [] for T in cases}
    for _ in range(reps):                            # alternating
        for T, call in cases.items():
            times[T].append(sample(call))
    for T in cases:
        nbytes = 4 * T * HW * C * 2
        s = _summary(times[T])
        print(json.dumps({"bench": "temporal_attention", "kernel": "16-frame" if T == 16 else "long", "B": 1, "T": T, "HW": HW, "heads": heads,
                          "device": torch.cuda.get_device_name(0), "reps": reps, "launches_per_sample": inner, "bytes": nbytes, **s,
                          "GB_per_s": round(nbytes / (s["median_ms"] * 1e-3) / 1e9, 1)}), flush=True)


def forward(T, reps):
    import torch
    from helpers import FULL, inp
    from moca_video_amd import UNetModel
    from moca_video_amd.weightgen import gen_state_dict
    torch.cuda.set_device(0)
    m = UNetModel(**FULL)
    m.load_state_dict(gen_state_dict({k: v.shape for k, v in m.state_dict().items()}, 11), strict=True)
    m = m.cuda()
    x = inp(f"bench_lf.x{T}", (1, 4, T, 40, 64)).cuda()
    ctx = [inp("bench_lf.ctx", (1, 77, 1024)).cuda(), inp("bench_lf.uctx", (1, 77, 1024)).cuda()]
    t, fps = torch.tensor([500]).cuda(), torch.tensor([10]).cuda()
    run = lambda: m.forward_segments(x, t, ctx, fps=[fps, fps], shared_x=True)
    for _ in range(4):                               # eager, capture, two replays
        run()
    torch.cuda.synchronize()
    assert any(p.graph is not None for p in m._plans.values()), "hipGraph replay path was not taken"
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    print(json.dumps({"bench": "shared_prefix_forward", "B": 2, "latents": [1, 4, T, 40, 64], "tokens": 77,
                      "device": torch.cuda.get_device_name(0), "reps": reps, **_summary(ms)}), flush=True)
    m._invalidate()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--only", choices=sorted(STEPS))
    ap.add_argument("--child", choices=sorted(STEPS), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps: a median of at least 20 samples")
    if a.child == "kernel":
        return kernel(a.reps, a.inner)
    if a.child:
        return forward(int(a.child[len("forward"):]), a.reps)
    for step in ([a.only] if a.only else list(STEPS)):
        cmd = ["timeout", "-k", "10", str(STEPS[step]), sys.executable, os.path.abspath(__file__), "--child", step,
               "--reps", str(a.reps), "--inner", str(a.inner)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            sys.exit(f"bench_long_frames: step {step} ended with status {rc}; nothing further is started")


if __name__ == "__main__":
    main()
