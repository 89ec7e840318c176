#!/usr/bin/env python3
"""Time of one `DDIMSampler.decode` step beside one `DDIMSampler.sample` step on the GPU, same model, same process:

  sample  S DDIM steps from x_T on the engine over all S schedule rows;
  decode  t_start steps from a noised latent on the engine over the first t_start rows (ddim.py:674-692).

Full-width UNet, x [1, 4, 16, 40, 64], 77 tokens, guidance 12: both are one replay of the same recorded launch sequence per step (the
truncated engine differs in the S its two sampler kernels index the tables with), so the expectation is equal per-step times.  Each
engine is built and captured first (warm-up run), then whole trajectories alternate; the time of a trajectory is taken between two
events around its steps and divided by their number.  One JSON line each.

    python tools/bench_v2v.py [--steps S] [--t-start K] [--reps N] [--reduced]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--t-start", type=int, default=6)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--reduced", action="store_true", help="the reduced-width UNet of the tests at [1, 4, 8, 16, 16]")
    a = ap.parse_args()
    from helpers import FULL, REDUCED, inp
    from moca_video_amd import DenoiseModel
    from moca_video_amd.fifo_graph import BaseEngine
    from moca_video_amd.sampler import DDIMSampler
    from moca_video_amd.weightgen import gen_state_dict
    torch.cuda.set_device(0)
    shape, dim = ((1, 4, 8, 16, 16), 128) if a.reduced else ((1, 4, 16, 40, 64), 1024)
    m = DenoiseModel({"target": UNET, "params": dict(REDUCED if a.reduced else FULL)})
    unet = m.model.diffusion_model
    unet.load_state_dict(gen_state_dict({k: v.shape for k, v in unet.state_dict().items()}, 11), strict=True)
    m = m.cuda()
    x = inp("bench_v2v.x", shape).cuda()
    cond = {"c_crossattn": [inp("bench_v2v.ctx", (1, 77, dim)).cuda()]}
    uc = {"c_crossattn": [inp("bench_v2v.uctx", (1, 77, dim)).cuda()]}
    s = DDIMSampler(m)
    s.make_schedule(a.steps, ddim_eta=1.0, verbose=False)
    # two engines side by side (the sampler's own cache holds one at a time): all rows / the first t_start rows
    engines = {"sample": (BaseEngine(m, s, x, cond, uc, 12.0, seed=1), a.steps),
               "decode": (BaseEngine(m, s, x, cond, uc, 12.0, seed=1, n_rows=a.t_start), a.t_start)}

    def run(name, seed):
        eng, n = engines[name]
        eng.reset(x, cond, uc, seed)
        if name == "decode":
            eng.encode(x, a.t_start)
        st = eng.plan.stream
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(n):
            eng.step()
        e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    for name in engines:                             # eager pass + capture + replays
        run(name, 0)
    times = {k: [] for k in engines}
    for r in range(a.reps):
        for name in engines:
            times[name].append(run(name, r + 1))
    for name, (eng, n) in engines.items():
        assert eng.plan.graph is not None
        print(json.dumps({"bench": "ddim_step", "path": name, "steps_per_trajectory": n, "table_rows": eng.S, "latents": list(shape),
                          "device": torch.cuda.get_device_name(0), "reps": a.reps,
                          "median_ms_per_step": round(statistics.median(times[name]), 4), "min_ms_per_step": round(min(times[name]), 4),
                          "max_ms_per_step": round(max(times[name]), 4)}), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
