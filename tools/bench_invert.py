#!/usr/bin/env python3
"""Time of one DDIM inversion step (`DDIMSampler.encode` on `fifo_graph.InvertEngine`: one hipGraph per step) beside one `decode` step of
the same build in the same run, and beside the UNet forwards they contain, same model, same process:

  invert_step          unguided, B = 1: [timestep rows] + forward + [moca_base_ddim_step_f32, eps_u NULL, zero noise]
  invert_step_guided   guidance: 2 B rows with the shared prefix
  decode_step_guided   `fifo_graph.BaseEngine` (the step of `sample` / `decode`): the same with a Philox draw in front
  forward_b1           `UNetModel.forward` of the same B = 1 plan shape            } what a step is expected to cost: a forward, one or
  forward_b2_shared    `forward_segments(shared_x=True)` of the same 2 B plan shape } two small launches in front, one elementwise pass behind

(an unguided `decode` step has no one-graph form -- `BaseEngine.supported` refuses guidance 1 -- so there is no fourth engine.)

Full-width UNet, x [1, 4, 16, 40, 64], 77 tokens.  Every path is built and captured first (eager pass, capture, replay), then samples of
`--steps` back-to-back steps alternate between the paths; a sample's time is taken between two events on the stream that runs it and
divided by the number of steps.  One JSON line each, the median over `--reps` samples, then the differences the expectation is about.

    python tools/bench_invert.py [--steps N] [--reps N] [--reduced]"""
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
    from moca_video_amd.fifo_graph import BaseEngine, InvertEngine
    from moca_video_amd.sampler import DDIMSampler
    from moca_video_amd.weightgen import gen_state_dict
    torch.cuda.set_device(0)
    shape, dim = ((1, 4, 8, 16, 16), 128) if a.reduced else ((1, 4, 16, 40, 64), 1024)
    m = DenoiseModel({"target": UNET, "params": dict(REDUCED if a.reduced else FULL)})
    unet = m.model.diffusion_model
    unet.load_state_dict(gen_state_dict({k: v.shape for k, v in unet.state_dict().items()}, 11), strict=True)
    m = m.cuda()
    x = inp("bench_invert.x", shape).cuda()
    fps = torch.tensor([10]).cuda()
    cond = {"c_crossattn": [inp("bench_invert.ctx", (1, 77, dim)).cuda()], "fps": fps}
    uc = {"c_crossattn": [inp("bench_invert.uctx", (1, 77, dim)).cuda()], "fps": fps}
    S = a.steps
    sampler = DDIMSampler(m)
    sampler.make_schedule(S, ddim_eta=0.0, verbose=False)
    engines = {"invert_step": InvertEngine(m, sampler, x, cond),
               "invert_step_guided": InvertEngine(m, sampler, x, cond, uc, 7.5),
               "decode_step_guided": BaseEngine(m, sampler, x, cond, uc, 7.5, seed=1)}
    resets = {"invert_step": lambda e, seed: e.reset(x, cond), "invert_step_guided": lambda e, seed: e.reset(x, cond, uc),
              "decode_step_guided": lambda e, seed: e.reset(x, cond, uc, seed)}
    t = torch.tensor([500]).cuda()
    ctxs = [cond["c_crossattn"][0], uc["c_crossattn"][0]]
    forwards = {"forward_b1": lambda: unet(x, t, context=ctxs[0], fps=fps),
                "forward_b2_shared": lambda: unet.forward_segments(x, t, ctxs, fps=[fps, fps], shared_x=True)}

    def run(name, seed):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if name in engines:
            eng = engines[name]
            resets[name](eng, seed)
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
        print(json.dumps({"bench": "invert_step", "path": name, "steps_per_sample": S, "latents": list(shape), "tokens": 77,
                          "device": torch.cuda.get_device_name(0), "reps": a.reps, "median_ms_per_step": round(med[name], 4),
                          "min_ms_per_step": round(min(times[name]), 4), "max_ms_per_step": round(max(times[name]), 4)}), flush=True)
    d = lambda p, q: round(med[p] - med[q], 4)
    print(json.dumps({"bench": "invert_step_differences_ms", "invert_minus_forward_b1": d("invert_step", "forward_b1"),
                      "invert_guided_minus_forward_b2_shared": d("invert_step_guided", "forward_b2_shared"),
                      "invert_guided_minus_decode_guided": d("invert_step_guided", "decode_step_guided")}), flush=True)
    for e in engines.values():
        e.close()


if __name__ == "__main__":
    main()
