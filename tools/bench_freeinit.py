#!/usr/bin/env python3
"""What a FreeInit iteration boundary costs on the GPU: the wall time of `DDIMSampler.sample_freeinit` (num_iters trajectories on one
step graph, `BaseEngine.reinit` between them) beside `DDIMSampler.sample` -- the base 'N DDIM steps' path, unchanged by FreeInit --
in the same process, on the same cached engine.

Full-width UNet, x [1, 4, 16, 40, 64], 77 tokens, guidance 12, 2 iterations x 10 steps.  Both paths run once first (engine build, eager
pass, capture), then alternate; a run is timed on the host between two device synchronisations, read-back included.

  base       sample(S = 10)                                  one trajectory
  freeinit   sample_freeinit([10, 10])                       two trajectories + one boundary
  fast       sample_freeinit([5, 10])  (use_fast_sampling)   set_schedule instead of a second capture
  reinit     BaseEngine.reinit alone, between two events on the plan's stream

boundary = (freeinit - num_iters x base) / (num_iters - 1): a boundary replaces one `reset` + read-back of the base path by one
`reinit`, so it can come out below zero.  `captures` counts engines built during the timed runs (expected: 0).  One JSON line each.

    python tools/bench_freeinit.py [--steps S] [--iters K] [--reps N] [--reduced]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
UNET = "lvdm.modules.networks.openaimodel3d.UNetModel"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--reduced", action="store_true", help="the reduced-width UNet of the tests at [1, 4, 8, 16, 16]")
    a = ap.parse_args()
    from helpers import FULL, REDUCED, inp
    from moca_video_amd import DenoiseModel
    from moca_video_amd.fifo_graph import BaseEngine
    from moca_video_amd.freeinit import freeinit_steps, get_freq_filter
    from moca_video_amd.sampler import DDIMSampler
    from moca_video_amd.weightgen import gen_state_dict
    torch.cuda.set_device(0)
    shape, dim = ((1, 4, 8, 16, 16), 128) if a.reduced else ((1, 4, 16, 40, 64), 1024)
    m = DenoiseModel({"target": UNET, "params": dict(REDUCED if a.reduced else FULL)})
    unet = m.model.diffusion_model
    unet.load_state_dict(gen_state_dict({k: v.shape for k, v in unet.state_dict().items()}, 11), strict=True)
    m = m.cuda()
    x_T = inp("bench_freeinit.x", shape).cuda()
    cond = {"c_crossattn": [inp("bench_freeinit.ctx", (1, 77, dim)).cuda()]}
    uc = {"c_crossattn": [inp("bench_freeinit.uctx", (1, 77, dim)).cuda()]}
    lpf = get_freq_filter(shape, "cuda", "butterworth", 4, 0.25, 0.25)
    s = DDIMSampler(m)
    kw = dict(conditioning=cond, eta=1.0, x_T=x_T, unconditional_guidance_scale=12.0, unconditional_conditioning=uc)
    plans = {"base": None, "freeinit": freeinit_steps(a.steps, a.iters, False), "fast": freeinit_steps(a.steps, a.iters, True)}
    built = []
    real_init = BaseEngine.__init__

    def counting(self, *args, **kwargs):
        built.append(1)
        real_init(self, *args, **kwargs)
    BaseEngine.__init__ = counting

    def run(name):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if plans[name] is None:
            out, _ = s.sample(S=a.steps, batch_size=shape[0], shape=shape[1:], **kw)
        else:
            out, _ = s.sample_freeinit(plans[name], shape[0], shape[1:], lpf, **kw)
        torch.cuda.synchronize()
        assert torch.isfinite(out).all()
        return (time.perf_counter() - t0) * 1e3

    for name in plans:                               # engine build + eager pass + capture, and the filter / reinit buffers
        run(name)
    assert len(built) == 1, "base and FreeInit runs share one cached engine"
    eng = s._base_engine[1]
    graph = eng.plan.graph
    assert graph is not None
    times = {k: [] for k in plans}
    for _ in range(a.reps):
        for name in plans:
            times[name].append(run(name))
    assert eng.plan.graph is graph and s._base_engine[1] is eng
    re_ms = []
    for r in range(a.reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(eng.plan.stream)
        eng.reinit(x_T, lpf, seed=r)
        e1.record(eng.plan.stream)
        e1.synchronize()
        re_ms.append(e0.elapsed_time(e1))
    med = {k: statistics.median(v) for k, v in times.items()}
    common = {"latents": list(shape), "device": torch.cuda.get_device_name(0), "reps": a.reps, "guidance": 12.0}
    for name in plans:
        steps = [a.steps] if plans[name] is None else plans[name]
        print(json.dumps({"bench": "freeinit", "path": name, "steps": steps, "median_ms": round(med[name], 3),
                          "min_ms": round(min(times[name]), 3), "max_ms": round(max(times[name]), 3),
                          "ms_per_step": round(med[name] / sum(steps), 4), **common}), flush=True)
    bound = (med["freeinit"] - a.iters * med["base"]) / max(a.iters - 1, 1)
    print(json.dumps({"bench": "freeinit", "path": "boundary", "iterations": a.iters,
                      "boundary_ms_vs_base_runs": round(bound, 3), "reinit_alone_median_ms": round(statistics.median(re_ms[1:]), 4),
                      "reinit_alone_min_ms": round(min(re_ms[1:]), 4), "reinit_alone_max_ms": round(max(re_ms[1:]), 4),
                      "captures_in_timed_runs": len(built) - 1, "same_graph_after_fast_runs": True, **common}), flush=True)
    s.release()


if __name__ == "__main__":
    main()
