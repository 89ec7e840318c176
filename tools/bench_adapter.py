#!/usr/bin/env python3
"""Cost of the adapter maps in the B = 2 guidance step: the full-width UNet's shared-prefix forward of one latent video
[1, 4, 16, 40, 64] with the conditional and the unconditional 77-token context (`forward_segments(shared_x=True)`: the UNet part of
one DDIM step with classifier-free guidance), without and with the four `features_adapter` maps, in one process, alternating, after
a warm-up that covers the eager pass and the capture; median, minimum and maximum over the repetitions, one JSON line each.

What the maps add: four nchw_add_rows launches, and the statistics passes of the consumers of the summed maps (their producers no
longer leave GroupNorm statistics behind: DESIGN 3).  The plan without maps records the launches it recorded before the feature.

    python tools/bench_adapter.py [--reps N] [--warmup W] [--inner K] [--out profiles/adapter_step_cost.txt]

`--plain-only [--root DIR] [--label NAME]` times the forward without maps alone, with the package taken from the checkout DIR
(default: this one), and appends its line to `--out`: run against a checkout of the commit before the feature and against this one,
processes alternating, it shows whether the step without maps moved (the recorded launches are the same)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    ap.add_argument("--out", default=None)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--label", default=None)
    a = ap.parse_args()
    if a.root != ROOT and not a.plain_only:
        ap.error("--root goes with --plain-only: the maps need this checkout's plan")
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))
    from helpers import FULL, inp
    import moca_video_amd
    from moca_video_amd import UNetModel
    assert os.path.abspath(moca_video_amd.__file__).startswith(root + os.sep), moca_video_amd.__file__
    from moca_video_amd.weightgen import gen_state_dict
    torch.cuda.set_device(0)
    m = UNetModel(**FULL)
    m.load_state_dict(gen_state_dict({k: v.shape for k, v in m.state_dict().items()}, 11), strict=True)
    m = m.cuda()
    x = inp("bench_adapter.x", (1, 4, 16, 40, 64)).cuda()
    cc, cu = inp("bench_adapter.ctx", (1, 77, 1024)).cuda(), inp("bench_adapter.uctx", (1, 77, 1024)).cuda()
    t, fps = torch.tensor([500]).cuda(), torch.tensor([10]).cuda()
    calls = {"plain": lambda: m.forward_segments(x, t, [cc, cu], fps=[fps, fps], shared_x=True)}
    if not a.plain_only:
        import adapter_ref as AR
        maps = [f.cuda() for f in AR.features("bench_adapter", "step", 16, AR.sites(320, [1, 2, 4, 4], 40, 64), [3.6, 6.8, 11.0, 19.0])]
        calls["adapter"] = lambda: m.forward_segments(x, t, [cc, cu], fps=[fps, fps], shared_x=True, features_adapter=maps)
    for f in calls.values():
        timed(f, max(a.warmup, 3))            # eager pass, capture pass, replays
    times = {k: [] for k in calls}
    for _ in range(a.reps):
        for k, f in calls.items():
            times[k].append(timed(f, a.inner))
    lines = []
    for k in calls:
        plan = [p for key, p in m._plans.items() if (key[-1] == "adapter") == (k == "adapter")][0]
        lines.append(json.dumps({"bench": "unet_cfg_step", **({"tree": a.label or root} if a.plain_only else {}),
                                 "features_adapter": k == "adapter", "latents": [1, 4, 16, 40, 64], "branches": 2,
                                 "context_tokens": 77, "launches": len(plan.steps), "device": torch.cuda.get_device_name(0), "reps": a.reps,
                                 "inner": a.inner, "warmup": max(a.warmup, 3), "median_ms": round(statistics.median(times[k]), 4),
                                 "min_ms": round(min(times[k]), 4), "max_ms": round(max(times[k]), 4)}))
    if not a.plain_only:
        d = statistics.median(times["adapter"]) - statistics.median(times["plain"])
        lines.append(json.dumps({"bench": "unet_cfg_step", "adapter_minus_plain_median_ms": round(d, 4)}))
    print("\n".join(lines), flush=True)
    if a.out and a.plain_only:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    elif a.out:
        with open(a.out, "w") as f:
            f.write("# tools/bench_adapter.py: B = 2 guidance step (shared prefix), full-width UNet, without / with the four adapter maps;\n"
                    "# alternating in one process, ms per forward\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
