#!/usr/bin/env python3
"""Time of one masked step of DDIM / DPM-Solver inpainting beside the unmasked step it extends, same model, same process, guided
(2 B rows with the shared prefix):

  base_step           `fifo_graph.BaseEngine`: [timestep rows, Philox draw] + forward + [moca_base_ddim_step_f32]
  base_step_masked    the same with a mask: the Philox launch covers [noise | noise_q], then the blend (moca_ddpm_step_f32 without eps) in front of the forward
  dpm_step            `fifo_graph.DpmEngine`: [timestep rows] + forward + [the multistep step]; nothing is drawn
  dpm_step_masked     the same with a mask: one Philox launch over noise_q and the blend
  blend_alone         the blend launch by itself on the same buffers, back to back: the separate launch's own time

Full-width UNet, x [1, 4, 16, 40, 64], 77 tokens.  Every engine is built and captured first (eager pass, capture, replay), then samples
of `--steps` back-to-back steps alternate between the paths; a sample's time is taken between two events on the stream that runs it
and divided by the number of steps.  One JSON line each: the median over `--reps` samples with the spread (min, max), then the
differences the expectation is about (one more draw and one elementwise pass should sit inside the unmasked step's spread).

    python tools/bench_inpaint.py [--steps N] [--reps N] [--reduced]"""
import argparse
import ctypes as C
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
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--reduced", action="store_true", help="the reduced-width UNet of the tests at [1, 4, 8, 16, 16]")
    a = ap.parse_args()
    from helpers import FULL, REDUCED, inp
    from moca_video_amd import DenoiseModel
    from moca_video_amd import lib as L
    from moca_video_amd.fifo_graph import BaseEngine, DpmEngine
    from moca_video_amd.sampler import DDIMSampler, DPMSolverSampler
    from moca_video_amd.weightgen import gen_state_dict
    torch.cuda.set_device(0)
    shape, dim = ((1, 4, 8, 16, 16), 128) if a.reduced else ((1, 4, 16, 40, 64), 1024)
    m = DenoiseModel({"target": UNET, "params": dict(REDUCED if a.reduced else FULL)})
    unet = m.model.diffusion_model
    unet.load_state_dict(gen_state_dict({k: v.shape for k, v in unet.state_dict().items()}, 11), strict=True)
    m = m.cuda()
    x, x0 = inp("bench_inpaint.x", shape).cuda(), inp("bench_inpaint.x0", shape).cuda()
    mask = torch.zeros((1, 1) + shape[2:]).cuda()
    mask[..., : shape[-1] // 2] = 1.0
    fps = torch.tensor([10]).cuda()
    cond = {"c_crossattn": [inp("bench_inpaint.ctx", (1, 77, dim)).cuda()], "fps": fps}
    uc = {"c_crossattn": [inp("bench_inpaint.uctx", (1, 77, dim)).cuda()], "fps": fps}
    S = a.steps
    ddim, dpm = DDIMSampler(m), DPMSolverSampler(m)
    ddim.make_schedule(S, ddim_eta=1.0, verbose=False)
    dpm.make_schedule(S + 1, verbose=False)                          # (the row at timestep 0 is not stepped: S stepped rows)
    mk = dict(mask=mask, x0=x0)
    engines = {"base_step": BaseEngine(m, ddim, x, cond, uc, 7.5, seed=1), "base_step_masked": BaseEngine(m, ddim, x, cond, uc, 7.5, seed=1, **mk),
               "dpm_step": DpmEngine(m, dpm, x, cond, uc, 7.5, seed=1), "dpm_step_masked": DpmEngine(m, dpm, x, cond, uc, 7.5, seed=1, **mk)}
    be = engines["base_step_masked"]

    blend = be._blend_launch()                           # the launch the masked engine records, on its own buffers

    def blend_alone():
        blend(L.load(), None, C.c_void_p(torch.cuda.current_stream().cuda_stream))

    def run(name, seed):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if name in engines:
            eng = engines[name]
            eng.reset(x, cond, uc, seed, **(mk if eng.masked else {}))
            st = eng.plan.stream
            e0.record(st)
            for _ in range(S):
                eng.step()
            e1.record(st)
        else:
            be.sync_to()
            torch.cuda.synchronize()
            e0.record()
            for _ in range(S):
                blend_alone()
            e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / S

    names = list(engines) + ["blend_alone"]
    for name in names:                               # eager pass + capture + replays
        run(name, 0)
    assert all(e.plan.graph is not None for e in engines.values())
    times = {k: [] for k in names}
    for r in range(a.reps):
        for name in names:
            times[name].append(run(name, r + 1))
    med = {k: statistics.median(v) for k, v in times.items()}
    for name in names:
        print(json.dumps({"bench": "inpaint_step", "path": name, "steps_per_sample": S, "latents": list(shape), "tokens": 77,
                          "device": torch.cuda.get_device_name(0), "reps": a.reps, "median_ms_per_step": round(med[name], 4),
                          "min_ms_per_step": round(min(times[name]), 4), "max_ms_per_step": round(max(times[name]), 4)}), flush=True)
    d = lambda p, q: round(med[p] - med[q], 4)
    spread = lambda p: round(max(times[p]) - min(times[p]), 4)
    print(json.dumps({"bench": "inpaint_step_differences_ms", "mask_base": d("base_step_masked", "base_step"), "base_step_spread": spread("base_step"),
                      "mask_dpm": d("dpm_step_masked", "dpm_step"), "dpm_step_spread": spread("dpm_step"),
                      "blend_alone": round(med["blend_alone"], 4)}), flush=True)
    for e in engines.values():
        e.close()


if __name__ == "__main__":
    main()
