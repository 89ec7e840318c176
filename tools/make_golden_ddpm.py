#!/usr/bin/env python3
"""Generate the DDPM-sampler goldens by running the REAL reference methods (lvdm/models/ddpm3d.py) on the CPU, as unbound functions on a
stand-in `nn.Module` (the way tools/make_golden_v2v.py borrows `apply_model`): `DDPM.register_schedule` (:113-165),
`predict_start_from_noise` (:212-216), `q_posterior` (:218-225) and `LatentDiffusion.q_sample` (:412-420), `p_mean_variance`
(:565-588), `p_sample` (:591-610), `p_sample_loop` (:613-657), `apply_model` (:512-527).

  ddpm_tables.npz    the seven posterior tables of `register_schedule` for the YAML's schedule (1000, 0.00085, 0.012) and for the
                     fixture's (8, 0.05, 0.6).
  ddpm_methods.npz   the per-step methods at B = 2, t = [7, 0] on the fixture stand-in: q_sample with and without use_scale,
                     predict_start_from_noise, q_posterior, p_mean_variance(return_x0=True) with and without clip_denoised,
                     p_sample(return_x0=True).  The model output is a named tensor here (`EpsStub` in the wrapper's place), so these
                     hold fp32 sampler arithmetic only and are compared at 2e-6.
  ddpm_loop.npz      `p_sample_loop` over the real reduced-width UNet inside the real `DiffusionWrapper` (weights seed 11, loop_base's
                     context and fps 10) from a named x_T with named draws, shape [1,4,8,16,16]: plain (with the intermediates of
                     log_every_t = 3), clip_denoised, masked (half-ones mask [1,1,8,16,16], named x0), timesteps = 7, start_T = 5, and the
                     guidance extension (the real loop over an `apply_model` that composes the real one twice by ddim.py:304).
                     Fixture sensitivity, measured with the reference itself and ASSERTED here: dropping one table row (timesteps = 7),
                     clip_denoised and the mask must each move the result by more than 3 x TOL_BASE of max|ref|.  What a UNet timestep
                     that is off by one moves is measured and printed only: it is BELOW TOL_BASE, which is why the tests check the
                     timesteps handed to the UNet exactly.

    python tools/make_golden_ddpm.py

The stand-in's schedule (timesteps = 8, linear_start = 0.05, linear_end = 0.6, use_scale, mid_step = 4) makes `alphas_cumprod` run
from 0.95 to 0.053: the YAML's 1000-step schedule is useless for a short loop (at t < 8 a DDPM step barely moves x).

Same recipe as tools/make_golden.py (whose helpers it imports): parameters and inputs are regenerated bit-identically from
moca_video_amd.weightgen by name, so a fixture holds only the expected outputs and the call metadata."""
import os
import sys
import time
from functools import partial

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as MG  # noqa: E402

sys.path.insert(0, os.path.join(MG.ROOT, "tests"))
from ddpm_ref import FIX, GUIDE_SCALE, LOOP_SHAPE, METHOD_SHAPE, METHOD_T, TABLE_NAMES, half_mask  # noqa: E402
from test_loops_gpu import TOL_BASE  # noqa: E402

FACTOR = 3.0                      # sensitivity margin over TOL_BASE


def relerr(got, ref):
    return ((got - ref).abs().max() / ref.abs().max()).item()


def stand_in_class(ddpm3d):
    DDPM, LD = ddpm3d.DDPM, ddpm3d.LatentDiffusion

    class StandIn(torch.nn.Module):
        """the attributes the borrowed methods read (ddpm3d.py:64-108,362-390), set as the reference's constructors set them"""
        register_schedule = DDPM.register_schedule
        predict_start_from_noise = DDPM.predict_start_from_noise
        q_posterior = DDPM.q_posterior
        q_sample = LD.q_sample
        p_mean_variance = LD.p_mean_variance
        p_sample = LD.p_sample
        p_sample_loop = LD.p_sample_loop
        apply_model = LD.apply_model

        def __init__(self, wrapper=None, timesteps=1000, linear_start=0.00085, linear_end=0.012, use_scale=True, scale_a=1, scale_b=0.7,
                     mid_step=400, parameterization="eps"):
            super().__init__()
            self.parameterization = parameterization
            self.v_posterior = 0.
            self.log_every_t = 100
            self.clip_denoised = False
            self.shorten_cond_schedule = False
            self.model = wrapper
            self.register_schedule(beta_schedule="linear", timesteps=timesteps, linear_start=linear_start, linear_end=linear_end)
            self.use_scale = use_scale
            if use_scale:                                                        # :363-376 (the "bug" branch)
                scale_arr = np.concatenate((np.linspace(scale_a, scale_b, mid_step), np.full(self.num_timesteps, scale_b)))
                self.register_buffer('scale_arr', partial(torch.tensor, dtype=torch.float32)(scale_arr))

    return StandIn


def tables_case(StandIn):
    out = {}
    for tag, kw in (("default", {}), ("fix", FIX)):
        m = StandIn(**{k: v for k, v in kw.items() if k in ("timesteps", "linear_start", "linear_end")})
        for n in TABLE_NAMES:
            out[f"{tag}__{n}"] = getattr(m, n)
        print(f"[ddpm] tables {tag}: {m.num_timesteps} rows, alphas_cumprod {m.alphas_cumprod[0]:.3f} .. {m.alphas_cumprod[-1]:.3f}")
    MG.save("ddpm_tables", **out)


class Draws:
    """`noise_like` (p_sample, :601) and `torch.randn_like` (q_sample's default, :413) return the queued named tensors"""

    def __init__(self, ddpm3d, noises=(), mask_noises=()):
        self.mod, self.noises, self.mask_noises = ddpm3d, list(noises), list(mask_noises)

    def __enter__(self):
        self.real = (self.mod.noise_like, torch.randn_like)
        self.mod.noise_like = lambda shape, device, repeat=False: self.noises.pop(0).clone()
        torch.randn_like = lambda t, *a, **k: self.mask_noises.pop(0).clone()
        return self

    def __exit__(self, *exc):
        self.mod.noise_like, torch.randn_like = self.real


def build_wrapper(ddpm3d):
    wrapper = ddpm3d.DiffusionWrapper({"target": "lvdm.modules.networks.openaimodel3d.UNetModel", "params": dict(MG.REDUCED)},
                                      "crossattn").eval()
    MG.fill(wrapper.diffusion_model, 11)
    return wrapper


class EpsStub(torch.nn.Module):
    """in the `DiffusionWrapper`'s place for the per-step methods: the model output is a named tensor, so that these goldens hold fp32
    sampler arithmetic only (the loop's goldens run the real UNet)"""
    conditioning_key = "crossattn"

    def __init__(self, eps):
        super().__init__()
        self.eps = eps

    def forward(self, x, t, c_crossattn=None, **kw):
        assert x.shape == self.eps.shape and len(c_crossattn) == 1
        return self.eps.clone()


def methods_case(ddpm3d, StandIn):
    m = StandIn(EpsStub(MG.inp("ddpm.m.eps", METHOD_SHAPE)), **FIX)
    t = torch.tensor(METHOD_T)
    x, a, b = (MG.inp(f"ddpm.m.{n}", METHOD_SHAPE) for n in ("x", "a", "b"))
    cond = MG.inp("loop.ctx1", (1, 77, 128)).expand(2, -1, -1)                   # a tensor: apply_model makes it {"c_crossattn": [cond]}
    out = {}
    with torch.no_grad():
        out["q_sample"] = m.q_sample(x, t, noise=a)
        m.use_scale = False
        out["q_sample_noscale"] = m.q_sample(x, t, noise=a)
        m.use_scale = True
        out["predict_start"] = m.predict_start_from_noise(x, t, a)
        out["qp_mean"], out["qp_var"], out["qp_logvar"] = m.q_posterior(a, x, t)
        for tag, clip in (("pmv", False), ("pmv_clip", True)):
            out[tag + "_mean"], out[tag + "_var"], out[tag + "_logvar"], out[tag + "_x0"] = m.p_mean_variance(x, cond, t, clip, return_x0=True)
        with Draws(ddpm3d, [b]):
            out["p_sample"], out["p_sample_x0"] = m.p_sample(x, cond, t, return_x0=True)
    frac = ((out["pmv_x0"] != out["pmv_clip_x0"]).float().mean()).item()
    print(f"[ddpm] methods: clip_denoised changes {100 * frac:.0f} % of x_recon; p_sample t == 0 row is its mean: "
          f"{torch.equal(out['p_sample'][1], out['pmv_mean'][1])}")
    assert frac > 0.05 and torch.equal(out["p_sample"][1], out["pmv_mean"][1])
    MG.save("ddpm_methods", **out)


def loop_case(ddpm3d, StandIn, wrapper):
    m = StandIn(wrapper, **FIX)
    T = FIX["timesteps"]
    cond = {"c_crossattn": [MG.inp("loop.ctx1", (1, 77, 128))], "fps": torch.tensor([10])}
    uc = {"c_crossattn": [MG.inp("loop.uctx", (1, 77, 128))], "fps": torch.tensor([10])}
    x_T, x0 = MG.inp("ddpm.x_T", LOOP_SHAPE), MG.inp("ddpm.x0", LOOP_SHAPE)
    noises = [MG.inp(f"ddpm.noise{k}", LOOP_SHAPE) for k in range(T)]
    mnoises = [MG.inp(f"ddpm.mnoise{k}", LOOP_SHAPE) for k in range(T)]
    mask = half_mask()

    def run(model=m, masked=False, shift_t=0, **kw):
        d = Draws(ddpm3d, noises, mnoises if masked else ())
        real = model.apply_model
        if shift_t:
            model.apply_model = lambda x, t, c, **k: real(x, (t + shift_t).clamp(0, T - 1), c, **k)
        try:
            with torch.no_grad(), d:
                out = model.p_sample_loop(cond, LOOP_SHAPE, x_T=x_T, verbose=False, **(dict(mask=mask, x0=x0) if masked else {}), **kw)
        finally:
            if shift_t:
                del model.apply_model
        return out, T - len(d.noises)

    t0 = time.time()
    plain, inter = run(return_intermediates=True, log_every_t=3)[0]
    print(f"[ddpm] plain loop: {time.time() - t0:.1f}s, x_T std {x_T.std():.3f} -> std {plain.std():.3f} max {plain.abs().max():.2f}; "
          f"{len(inter)} intermediates")
    assert len(inter) == 5 and torch.equal(inter[0], x_T) and torch.equal(inter[-1], plain)    # x_T, i = 7, 6, 3, 0
    m.clip_denoised = True
    clip = run()[0]
    m.clip_denoised = False
    masked = run(masked=True)[0]
    t7, n7 = run(timesteps=7)
    s5, n5 = run(start_T=5)
    assert (n7, n5) == (7, 5)

    class Guided(StandIn):
        """the extension's golden: the real loop over the real apply_model composed twice with ddim.py:304"""

        def apply_model(self, x, t, c, **kw):
            e_c = StandIn.apply_model(self, x, t, c, **kw)
            e_u = StandIn.apply_model(self, x, t, uc, **kw)
            return e_u + GUIDE_SCALE * (e_c - e_u)

    guided = run(model=Guided(wrapper, **FIX))[0]
    # ---- fixture sensitivity (the reference against itself)
    need = FACTOR * TOL_BASE
    moved = {"timesteps = 7": relerr(t7, plain), "clip_denoised": relerr(clip, plain), "half-ones mask": relerr(masked, plain)}
    for k, v in moved.items():
        print(f"[ddpm] sensitivity, {k}: the result moves by {v:.3e} of max|ref| (need > {need:.2e}, margin {v / need:.1f} x)")
    assert all(v > need for v in moved.values()), "the fixture does not separate these from TOL_BASE: change the fixture"
    off = relerr(run(shift_t=1)[0], plain)
    print(f"[ddpm] sensitivity, UNet timestep + 1: {off:.3e} of max|ref| (TOL_BASE {TOL_BASE:.1e}): "
          f"{'BELOW the bound -- the tests check the UNet timesteps exactly' if off < TOL_BASE else 'above the bound'}")
    print(f"[ddpm] guidance {GUIDE_SCALE}: moves the result by {relerr(guided, plain):.3e}; std {guided.std():.3f}")
    MG.save("ddpm_loop", plain=plain, inter=torch.stack(inter), clip=clip, masked=masked, t7=t7, start5=s5, guided=guided,
            sens=np.asarray(list(moved.values()) + [off]))


def main():
    torch.set_num_threads(16)
    MG.import_reference()
    from lvdm.models import ddpm3d
    StandIn = stand_in_class(ddpm3d)
    tables_case(StandIn)
    methods_case(ddpm3d, StandIn)
    wrapper = build_wrapper(ddpm3d)
    loop_case(ddpm3d, StandIn, wrapper)


if __name__ == "__main__":
    main()
