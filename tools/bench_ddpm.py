#!/usr/bin/env python3
"""Time of one DDPM step (`DenoiseModel.p_sample_loop` on `fifo_graph.DdpmEngine`: one hipGraph per step) beside the UNet forward it
contains, same model, same process:

  ddpm_step           unguided, B = 1: [timestep rows, Philox draw] + forward + [moca_ddpm_step_f32]
  ddpm_step_masked    the same with a mask: one more Philox draw and the blend inside the same step kernel
  ddpm_step_guided    guidance: 2 B rows with the shared prefix
  ddpm_step_guided_masked
  forward_b1          `UNetModel.forward` of the same B = 1 plan shape            } the floor: a step is a forward, two or three small
  forward_b2_shared   `forward_segments(shared_x=True)` of the same 2 B plan shape } launches in front and one elementwise pass behind

Full-width UNet, x [1, 4, 16, 40, 64], 77 tokens.  Every path is built and captured first (eager pass, capture, replay), then samples of
`--steps` back-to-back steps alternate between the paths; a sample's time is taken between two events on the stream that runs it and
divided by the number of steps.  One JSON line each, the median over `--reps` samples, then the differences the expectation is about.

    python tools/bench_ddpm.py [--steps N] [--reps N] [--reduced]"""
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
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--reduced", action="store_true", help="the reduced-width UNet of the tests at [1, 4, 8, 16, 16]")
    a = ap.parse_args()
    from helpers import FULL, REDUCED, inp
    from moca_video_amd import DenoiseModel
    from moca_video_amd.fifo_graph import DdpmEngine
    from moca_video_amd.weightgen import gen_state_dict
    torch.cuda.set_device(0)
    shape, dim = ((1, 4, 8, 16, 16), 128) if a.reduced else ((1, 4, 16, 40, 64), 1024)
    m = DenoiseModel({"target": UNET, "params": dict(REDUCED if a.reduced else FULL)})
    unet = m.model.diffusion_model
    unet.load_state_dict(gen_state_dict({k: v.shape for k, v in unet.state_dict().items()}, 11), strict=True)
    m = m.cuda()
    x, x0 = inp("bench_ddpm.x", shape).cuda(), inp("bench_ddpm.x0", shape).cuda()
    mask = torch.zeros((1, 1) + shape[2:]).cuda()
    mask[..., : shape[-1] // 2] = 1.0
    fps = torch.tensor([10]).cuda()
    cond = {"c_crossattn": [inp("bench_ddpm.ctx", (1, 77, dim)).cuda()], "fps": fps}
    uc = {"c_crossattn": [inp("bench_ddpm.uctx", (1, 77, dim)).cuda()], "fps": fps}
    S = a.steps
    engines = {"ddpm_step": DdpmEngine(m, x, cond, None, 1.0, S, seed=1),
               "ddpm_step_masked": DdpmEngine(m, x, cond, None, 1.0, S, mask=mask, x0=x0, seed=1),
               "ddpm_step_guided": DdpmEngine(m, x, cond, uc, 7.5, S, seed=1),
               "ddpm_step_guided_masked": DdpmEngine(m, x, cond, uc, 7.5, S, mask=mask, x0=x0, seed=1)}
    t = torch.tensor([500]).cuda()
    ctxs = [cond["c_crossattn"][0], uc["c_crossattn"][0]]
    forwards = {"forward_b1": lambda: unet(x, t, context=ctxs[0], fps=fps),
                "forward_b2_shared": lambda: unet.forward_segments(x, t, ctxs, fps=[fps, fps], shared_x=True)}

    def run(name, seed):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if name in engines:
            eng = engines[name]
            masked = eng.masked
            eng.reset(x, cond, uc if eng.guided else None, seed, mask=mask if masked else None, x0=x0 if masked else None)
            st = eng.plan.stream
            e0.record(st)
            for _ in range(S):
                eng.step()
            e1.record(st)
        else:
            torch.cuda.synchronize()
            e0.record()
            for _ in range(S):
                forwards[name]()
            e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / S

    names = list(engines) + list(forwards)
    for name in names:                               # eager pass + capture + replays
        run(name, 0)
    assert all(e.plan.graph is not None for e in engines.values()) and sum(p.graph is not None for p in unet._plans.values()) >= 2
    times = {k: [] for k in names}
    for r in range(a.reps):
        for name in names:
            times[name].append(run(name, r + 1))
    med = {k: statistics.median(v) for k, v in times.items()}
    for name in names:
        print(json.dumps({"bench": "ddpm_step", "path": name, "steps_per_sample": S, "latents": list(shape), "tokens": 77,
                          "device": torch.cuda.get_device_name(0), "reps": a.reps, "median_ms_per_step": round(med[name], 4),
                          "min_ms_per_step": round(min(times[name]), 4), "max_ms_per_step": round(max(times[name]), 4)}), flush=True)
    d = lambda p, q: round(med[p] - med[q], 4)
    print(json.dumps({"bench": "ddpm_step_differences_ms", "step_minus_forward_b1": d("ddpm_step", "forward_b1"),
                      "guided_step_minus_forward_b2_shared": d("ddpm_step_guided", "forward_b2_shared"),
                      "mask_b1": d("ddpm_step_masked", "ddpm_step"), "mask_guided": d("ddpm_step_guided_masked", "ddpm_step_guided")}),
          flush=True)
    for e in engines.values():
        e.close()


if __name__ == "__main__":
    main()
