#!/usr/bin/env python3
"""Cost of a prompt switch in the one-graph FIFO loop (`FifoEngine.set_context`, fifo_ddim_sampling_multiprompts) at the headline
shape: full-width UNet, [1, 4, 16, 40, 64] windows, 4 partitions with lookahead (8 windows x CFG = one B = 16 forward per
iteration), 77-token prompts, masks handed in.  One engine; blocks of `inner` iterations with a switch every k in {1, 8}
iterations and with none, alternated on the same device, per-iteration time = HIP events on the engine's stream around the block
(median and min over `reps` blocks; profiles/multiprompt_switch_cost.txt).  Weights: bench.py's zero-data denoiser (random-init
weights drive the queue to overflow within ~50 iterations, see bench.ZeroDataDenoiser).

    python tools/bench_multiprompt.py [--reps N] [--inner M]"""
import argparse
import os
import statistics
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=8)
    a = ap.parse_args()
    import bench
    from moca_video_amd.fifo import prepare_latents
    from moca_video_amd.fifo_graph import FifoEngine
    from moca_video_amd.sampler import DDIMSampler
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    print(f"device: {torch.cuda.get_device_name(0)}")
    dm = bench.build_model(dev)
    bench.ZeroDataDenoiser(dm)
    T, H, W, S = 16, 40, 64, 64
    args = types.SimpleNamespace(num_inference_steps=S, video_length=T, lookahead_denoising=True, num_partitions=4, new_video_length=100)
    s = DDIMSampler(dm)
    s.make_schedule(S, ddim_eta=1.0, verbose=False)
    g = torch.Generator(device=dev).manual_seed(7)
    fps = torch.tensor([10], device=dev)
    prompts = [torch.randn(1, 77, 1024, device=dev, generator=g) for _ in range(2)]
    uc = {"c_crossattn": [torch.randn(1, 77, 1024, device=dev, generator=g)], "fps": fps}
    lat = prepare_latents(args, None, s, initial_latents=torch.randn(1, 4, T, H, W, device=dev, generator=g))
    Q = S + T // 2
    mask = torch.zeros(1, 1, Q, H, W, device=dev)
    mask[..., H // 4: 3 * H // 4, W // 4: 3 * W // 4] = 1.0
    cimg = torch.rand(1, 4, 1, H, W, device=dev, generator=g)
    eng = FifoEngine(args, dm, s, {"c_crossattn": [prompts[0]], "fps": fps}, uc, 12.0, lat, conditioned_image=cimg, masks=mask,
                     n_slots=8, seed=7)
    state = {"it": 0, "j": 0}

    def block(k):
        """`inner` iterations, switching the prompt before every k-th one (k = 0: never)"""
        a_, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(eng.plan.stream):
            a_.record()
        for _ in range(a.inner):
            if k and state["it"] % k == 0:
                state["j"] ^= 1
                eng.set_context(prompts[state["j"]])
            eng.step()
            state["it"] += 1
        with torch.cuda.stream(eng.plan.stream):
            b_.record()
        torch.cuda.synchronize()
        return a_.elapsed_time(b_) / a.inner
    for _ in range(3):                          # eager, capture, first replay
        eng.step()
    block(1)
    block(0)                                    # warm-up of both variants
    ks = (0, 1, 8)
    t = {k: [] for k in ks}
    for _ in range(a.reps):
        for k in ks:
            t[k].append(block(k))
    finite = bool(torch.isfinite(eng.latents()).all())
    graph_on = eng.plan.graph is not None and not eng.plan.graph_failed
    eng.close()
    base = statistics.median(t[0])
    print(f"FIFO iteration, B = 16 (8 windows x CFG), [1, 4, 16, 40, 64] windows, 77-token prompts, masks; {a.reps} alternating blocks "
          f"of {a.inner} iterations; one hipGraph throughout: {graph_on}; queue finite: {finite}")
    for k in ks:
        med = statistics.median(t[k])
        name = "no switch" if k == 0 else f"switch every {k}"
        print(f"  {name:16s} median {med:8.2f} ms  min {min(t[k]):8.2f} ms  max {max(t[k]):8.2f} ms  vs no switch {med / base - 1:+.3%}")


if __name__ == "__main__":
    main()
