#!/usr/bin/env python3
"""Generate the FreeInit goldens by running the REAL reference on the CPU: the FreeInit loop (Wu et al., 2023) is written HERE over the
reference's own `LatentDiffusion.q_sample` (lvdm/models/ddpm3d.py:412-420), `freq_mix_3d` / `get_freq_filter`
(utils/freeinit_utils.py) and `DDIMSampler.sample` (lvdm/models/samplers/ddim.py:109-252) -- the reference ships the utilities but no
loop that reaches them with T > 1.

    LPF = get_freq_filter(shape, filter_type, n, d_s, d_t)
    iteration 0 samples from the initial noise; iteration k >= 1 from
        freq_mix_3d(q_sample(samples_{k-1}, t = 999, noise = INITIAL noise), z_rand_k, LPF).reshape(shape)

  freeinit_reinit.npz  the re-initialisation alone (no UNet), 1000-step schedule: shape A [1,4,8,16,16] with all four filter types and,
                       for butterworth, a `use_scale` model (x scale_arr[999] = 0.7); shape B [2,4,16,16,24] (a batch the mix does
                       not squeeze, a DFT axis that is no power of two) with butterworth.  Named inputs `freeinit.{z0,init,zrand}.{A,B}`.
  freeinit_loop.npz    the trajectory: the real reduced-width UNet inside the real `DiffusionWrapper` through the real `apply_model`,
                       loop_base's contexts and fps, shape A, ddim_steps = 6, num_iters = 3, eta 1, guidance 12, use_scale, butterworth
                       (n 4, d_s = d_t 0.25); `full` = 6 steps per iteration, `fast` = coarse-to-fine [2, 4, 6].  Every iteration's start
                       (`x_T{k}`) and samples.  Two WRONG variants of iteration 1 of `full`, run with the reference too: (a) re-noised
                       with z_rand in place of the initial noise, (b) the filter applied without the fftshift (to the un-centred
                       spectrum).  ASSERTED here: each moves iteration 1's start by more than 10 x FREEINIT_TOL and its samples by
                       more than 10 x TOL_BASE of max|ref| -- a fixture that could not tell them apart would show nothing.

    python tools/make_golden_freeinit.py

Same recipe as tools/make_golden.py (whose helpers it imports): parameters and inputs are regenerated bit-identically from
moca_video_amd.weightgen by name, so a fixture holds only the expected outputs and the call metadata."""
import contextlib
import io
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as MG  # noqa: E402

sys.path.insert(0, os.path.join(MG.ROOT, "tests"))
from small_kernels_ref import FREEINIT_TOL  # noqa: E402
from test_loops_gpu import TOL_BASE  # noqa: E402

FACTOR = 10.0
SHAPE_A, SHAPE_B = (1, 4, 8, 16, 16), (2, 4, 16, 16, 24)
FILTERS = ("gaussian", "butterworth", "ideal", "box")
N, D_S, D_T = 4, 0.25, 0.25
DDIM_STEPS, NUM_ITERS, SCALE = 6, 3, 12.0
DIMS = (-3, -2, -1)


def relerr(got, ref):
    return ((got - ref).abs().max() / ref.abs().max()).item()


def steps_of(fast):
    """the loop's step counts (what moca_video_amd.freeinit.freeinit_steps returns)"""
    s = [max(1, int(DDIM_STEPS / NUM_ITERS * (k + 1))) if fast else DDIM_STEPS for k in range(NUM_ITERS)]
    s[-1] = DDIM_STEPS
    return s


def model_class(ddpm3d, wrapper=None):
    from lvdm.models.utils_diffusion import make_beta_schedule

    class Model(MG.FakeModel):
        """FakeModel + what the real `q_sample` reads, set as `register_schedule` sets it (ddpm3d.py:136-138)"""
        model = wrapper
        apply_model = ddpm3d.LatentDiffusion.apply_model
        q_sample = ddpm3d.LatentDiffusion.q_sample

        def __init__(self, use_scale=True):
            super().__init__()
            ac = np.cumprod(1. - make_beta_schedule("linear", 1000, linear_start=0.00085, linear_end=0.012), axis=0)
            self.sqrt_alphas_cumprod = torch.tensor(np.sqrt(ac), dtype=torch.float32)
            self.sqrt_one_minus_alphas_cumprod = torch.tensor(np.sqrt(1. - ac), dtype=torch.float32)
            self.use_scale = use_scale

    return Model


def reinit(FU, model, prev, initial_noise, z_rand, lpf, wrong=None):
    """the re-initialisation between two iterations, on the reference's functions; `wrong`: "a" re-noises with z_rand, "b" leaves the
    fftshift out (the centred filter meets the un-centred spectrum: the same as shifting the filter instead)"""
    t = torch.full((prev.shape[0],), model.num_timesteps - 1, dtype=torch.long)
    z_T = model.q_sample(prev, t, noise=z_rand if wrong == "a" else initial_noise)
    if wrong == "b":
        lpf = torch.fft.fftshift(lpf, dim=DIMS)
    return FU.freq_mix_3d(z_T.to(torch.float32), z_rand, lpf).reshape(prev.shape)


def reinit_case(FU, Model):
    out = {}
    plain, scaled = Model(use_scale=False), Model(use_scale=True)
    for tag, shape, filters in (("A", SHAPE_A, FILTERS), ("B", SHAPE_B, ("butterworth",))):
        z0, init, zr = (MG.inp(f"freeinit.{n}.{tag}", shape) for n in ("z0", "init", "zrand"))
        for ft in filters:
            lpf = FU.get_freq_filter(shape, "cpu", ft, N, D_S, D_T)
            out[f"{tag}_{ft}"] = reinit(FU, plain, z0, init, zr, lpf)
            if tag == "A" and ft == "butterworth":
                out[f"{tag}_{ft}_scale"] = reinit(FU, scaled, z0, init, zr, lpf)
        print(f"[freeinit] reinit {tag} {shape}: " + ", ".join(f"{k} std {v.std():.3f}" for k, v in out.items() if k.startswith(tag)))
    moved = relerr(out["A_butterworth_scale"], out["A_butterworth"])
    print(f"[freeinit] use_scale moves the re-initialised latents by {moved:.3e} of max|ref|")
    assert moved > FACTOR * FREEINIT_TOL
    MG.save("freeinit_reinit", n=np.asarray(N), d_s=np.asarray(D_S), d_t=np.asarray(D_T), **out)


def loop_case(FU, D, ddpm3d):
    wrapper = ddpm3d.DiffusionWrapper({"target": "lvdm.modules.networks.openaimodel3d.UNetModel", "params": dict(MG.REDUCED)},
                                      "crossattn").eval()
    MG.fill(wrapper.diffusion_model, 11)
    model = model_class(ddpm3d, wrapper)()
    fps = torch.tensor([10])
    cond = {"c_crossattn": [MG.inp("loop.ctx1", (1, 77, 128))], "fps": fps}
    uc = {"c_crossattn": [MG.inp("loop.uctx", (1, 77, 128))], "fps": fps}
    initial_noise = MG.inp("freeinit.x_T", SHAPE_A)
    z_rands = [MG.inp(f"freeinit.zrand{k}", SHAPE_A) for k in range(1, NUM_ITERS)]
    noises = [[MG.inp(f"freeinit.noise{k}.{i}", SHAPE_A) for i in range(DDIM_STEPS)] for k in range(NUM_ITERS)]
    lpf = FU.get_freq_filter(SHAPE_A, "cpu", "butterworth", N, D_S, D_T)
    real = D.noise_like

    def sample(x, S, k):
        q = list(noises[k][:S])
        D.noise_like = lambda shp, dev, repeat=False: q.pop(0).clone()
        try:
            with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
                s = D.DDIMSampler(model)
                out, _ = s.sample(S=S, conditioning=cond, batch_size=SHAPE_A[0], shape=SHAPE_A[1:], verbose=False,
                                  unconditional_guidance_scale=SCALE, unconditional_conditioning=uc, eta=1.0,
                                  temporal_length=SHAPE_A[2], conditional_guidance_scale_temporal=None, x_T=x)
        finally:
            D.noise_like = real
        assert not q, "sample drew another number of noises than steps"
        return out

    out = {}
    for mode, fast in (("full", False), ("fast", True)):
        steps = steps_of(fast)
        t0 = time.time()
        x = initial_noise
        for k, S in enumerate(steps):
            if k > 0:
                with torch.no_grad():
                    x = reinit(FU, model, out[f"{mode}_samples{k - 1}"], initial_noise, z_rands[k - 1], lpf)
                out[f"{mode}_x_T{k}"] = x
            out[f"{mode}_samples{k}"] = sample(x, S, k)
        out[f"{mode}_steps"] = np.asarray(steps)
        print(f"[freeinit] {mode} {steps}: {time.time() - t0:.1f}s, samples std " +
              ", ".join(f"{out[f'{mode}_samples{k}'].std():.3f}" for k in range(NUM_ITERS)))
    # ---- the two wrong variants of iteration 1 (the reference against itself)
    for w in ("a", "b"):
        with torch.no_grad():
            x = reinit(FU, model, out["full_samples0"], initial_noise, z_rands[0], lpf, wrong=w)
        out[f"full_x_T1_wrong_{w}"] = x
        out[f"full_samples1_wrong_{w}"] = sample(x, DDIM_STEPS, 1)
        mx, ms = relerr(x, out["full_x_T1"]), relerr(out[f"full_samples1_wrong_{w}"], out["full_samples1"])
        print(f"[freeinit] wrong variant ({w}): iteration 1 starts {mx:.3e} away (need > {FACTOR * FREEINIT_TOL:.1e}), its samples end "
              f"{ms:.3e} away (need > {FACTOR * TOL_BASE:.2e}) of max|ref|")
        assert mx > FACTOR * FREEINIT_TOL and ms > FACTOR * TOL_BASE, "the fixture does not separate this variant: change the fixture"
    MG.save("freeinit_loop", scale=np.asarray(SCALE), **out)


def main():
    torch.set_num_threads(16)
    MG.import_reference()
    from lvdm.models import ddpm3d
    from utils import freeinit_utils as FU
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from make_golden_v2v import patched_sampler_module
    D = patched_sampler_module()
    reinit_case(FU, model_class(ddpm3d))
    loop_case(FU, D, ddpm3d)


if __name__ == "__main__":
    main()
