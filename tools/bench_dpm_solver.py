#!/usr/bin/env python3
"""What a DPM-Solver++(2M) step costs beside a DDIM step, and what the solver's shorter trajectory buys, same model, same process:

  ddim_step_guided     `fifo_graph.BaseEngine` (the step of `DDIMSampler.sample`): [timestep rows, Philox draw] + forward + [DDIM update]
  dpm_step_guided      `fifo_graph.DpmEngine` (the step of `DPMSolverSampler.sample`): [timestep rows] + forward + [multistep update]
  base_ddim_sampling   50 steps, eta 0, on the step graph: engine built, captured and released inside the call, as a user runs it
  dpm_solver_sampling  20 schedule rows (19 forwards), the same

Expectation to test: the two steps cost the same within the run-to-run spread -- the multistep kernel reads and writes one more
fp32 stream of the latents' size (the history) than the DDIM update, against a UNet forward of two branches.

Full-width UNet, x [1, 4, 16, 40, 64], 77 tokens, guidance 7.5.  Both engines are built and captured first (eager pass, capture,
replay), then samples of `--steps` back-to-back steps alternate between them; a sample's time is taken between two events on the
stream that runs it and divided by the number of steps.  The drivers alternate too, timed by a host clock around a call that ends in a
device synchronise, after one untimed call each.  One JSON line per path (the median, the minimum and the maximum over the samples),
then the differences; the lines are also written to `--out` (default profiles/dpm_solver_step_cost.txt).

    python tools/bench_dpm_solver.py [--steps N] [--reps N] [--driver-reps N] [--reduced] [--out FILE]"""
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
SCALE = 7.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--driver-reps", type=int, default=3)
    ap.add_argument("--reduced", action="store_true", help="the reduced-width UNet of the tests at [1, 4, 8, 16, 16]")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dpm_solver_step_cost.txt"))
    a = ap.parse_args()
    from helpers import FULL, REDUCED, inp
    from moca_video_amd import DenoiseModel, dpm_solver_sampling
    from moca_video_amd.fifo import base_ddim_sampling
    from moca_video_amd.fifo_graph import BaseEngine, DpmEngine
    from moca_video_amd.sampler import DDIMSampler, DPMSolverSampler
    from moca_video_amd.weightgen import gen_state_dict
    assert torch.cuda.is_available(), "bench_dpm_solver measures on the GPU"
    torch.cuda.set_device(0)
    shape, dim = ((1, 4, 8, 16, 16), 128) if a.reduced else ((1, 4, 16, 40, 64), 1024)
    m = DenoiseModel({"target": UNET, "params": dict(REDUCED if a.reduced else FULL)})
    unet = m.model.diffusion_model
    unet.load_state_dict(gen_state_dict({k: v.shape for k, v in unet.state_dict().items()}, 11), strict=True)
    m = m.cuda()
    x = inp("bench_dpm.x", shape).cuda()
    fps = torch.tensor([10]).cuda()
    cond = {"c_crossattn": [inp("bench_dpm.ctx", (1, 77, dim)).cuda()], "fps": fps}
    uc_emb = inp("bench_dpm.uctx", (1, 77, dim)).cuda()
    uc = dict(cond, c_crossattn=[uc_emb])
    S = a.steps
    ddim, dpm = DDIMSampler(m), DPMSolverSampler(m)
    ddim.make_schedule(S + 1, ddim_eta=0.0, verbose=False)              # S + 1 rows: the solver steps S of them
    dpm.make_schedule(S + 1, verbose=False)
    engines = {"ddim_step_guided": BaseEngine(m, ddim, x, cond, uc, SCALE, seed=1), "dpm_step_guided": DpmEngine(m, dpm, x, cond, uc, SCALE)}
    assert engines["dpm_step_guided"].n_stepped == S
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    def run(name, seed):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        eng = engines[name]
        eng.reset(x, cond, uc, seed)
        st = eng.plan.stream
        e0.record(st)
        for _ in range(S):
            eng.step()
        e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1) / S

    for name in engines:                             # eager pass + capture + replays
        run(name, 0)
    assert all(e.plan.graph is not None for e in engines.values())
    times = {k: [] for k in engines}
    for r in range(a.reps):
        for name in engines:
            times[name].append(run(name, r + 1))
    med = {k: statistics.median(v) for k, v in times.items()}
    common = {"latents": list(shape), "tokens": 77, "cfg_scale": SCALE, "device": torch.cuda.get_device_name(0)}
    for name in engines:
        emit(dict({"bench": "dpm_solver_step", "path": name, "steps_per_sample": S, "reps": a.reps, "median_ms_per_step": round(med[name], 4),
                   "min_ms_per_step": round(min(times[name]), 4), "max_ms_per_step": round(max(times[name]), 4)}, **common))
    emit({"bench": "dpm_solver_step_difference_ms", "dpm_minus_ddim": round(med["dpm_step_guided"] - med["ddim_step_guided"], 4),
          "ddim_spread": round(max(times["ddim_step_guided"]) - min(times["ddim_step_guided"]), 4),
          "dpm_spread": round(max(times["dpm_step_guided"]) - min(times["dpm_step_guided"]), 4)})
    for e in engines.values():
        e.close()

    drivers = {"base_ddim_sampling": (50, lambda: base_ddim_sampling(m, cond, list(shape), 50, 0.0, SCALE, uc_emb=uc_emb, x_T=x)),
               "dpm_solver_sampling": (19, lambda: dpm_solver_sampling(m, cond, list(shape), steps=20, cfg_scale=SCALE, uc_emb=uc_emb, x_T=x))}

    def call(name):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = drivers[name][1]()[2]
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out).all())
        return (time.perf_counter() - t0) * 1e3

    for name in drivers:
        call(name)
    dt = {k: [] for k in drivers}
    for _ in range(a.driver_reps):
        for name in drivers:
            dt[name].append(call(name))
    for name in drivers:
        emit(dict({"bench": "dpm_solver_trajectory", "path": name, "forwards": drivers[name][0], "reps": a.driver_reps,
                   "median_ms": round(statistics.median(dt[name]), 2), "min_ms": round(min(dt[name]), 2), "max_ms": round(max(dt[name]), 2)}, **common))
    emit({"bench": "dpm_solver_trajectory_ratio", "ddim50_over_dpm20": round(statistics.median(dt["base_ddim_sampling"]) /
                                                                            statistics.median(dt["dpm_solver_sampling"]), 3)})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("tools/bench_dpm_solver.py" + (" --reduced" if a.reduced else "") + f" --steps {S} --reps {a.reps} --driver-reps {a.driver_reps}\n")
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
