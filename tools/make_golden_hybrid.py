#!/usr/bin/env python3
"""Generate the hybrid-conditioning goldens by running the REAL reference modules on CPU: the real `DiffusionWrapper`
(ddpm3d.py:696-763) around the real reduced-width `UNetModel` built with `in_channels = 4 + k`, weights `fill(model, 11)`.

  hybrid_wrapper.npz  key 'hybrid', in_channels 8, x [1,4,8,16,16], 77-token context:
                        a  one c_concat [1,4,8,16,16], uniform t = [500];
                        b  per-frame t (the is_fifo branch of the UNet);
                        c  B = 2, two c_concat entries of 2 channels each;
                        d  as a, with fps=tensor([10]) in the call: ASSERTED here to equal a bit for bit (the hybrid branch drops
                           **kwargs, ddpm3d.py:717), stored as the same array;
                        e  in_channels 9, c_concat of 4 + 1 channels, key 'hybrid-adm-mask', with s= and mask=;
                      plus `a_zero`: case a with c_concat replaced by zeros (the sensitivity condition: it must differ from a by more
                      than 20 x TOL_UNET in max-norm, else the c_concat INPUT is scaled up until it does; `concat_scale` records it).
  hybrid_sample.npz   the real `DDIMSampler.sample` on model a through the real `LatentDiffusion.apply_model`, with the settings of
                      loop_base (shape [1,4,8,16,16], S = 10, eta 1, guidance scale 12, use_scale, recorded x_T and per-step noise),
                      uc = copy of cond with another context: the final latents.
  unet_full_hybrid.npz  (--full) the YAML's UNet params with in_channels = 8, one 'hybrid' call at [1,8,16,40,64].

    python tools/make_golden_hybrid.py [--full]

Same recipe as tools/make_golden.py (whose helpers it imports): parameters and inputs are regenerated bit-identically from
moca_video_amd.weightgen by name, so a fixture holds only the expected outputs and the call metadata."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as MG  # noqa: E402

sys.path.insert(0, os.path.join(MG.ROOT, "tests"))
from test_unet_gpu import TOL_UNET  # noqa: E402

SENSITIVITY = 20 * TOL_UNET
UNET_TARGET = "lvdm.modules.networks.openaimodel3d.UNetModel"
SHAPE = (8, 16, 16)          # T, h, w


def relerr(got, ref):
    return ((got - ref).abs().max() / ref.abs().max()).item()


def wrapper_for(ddpm3d, params, key):
    w = ddpm3d.DiffusionWrapper({"target": UNET_TARGET, "params": dict(params)}, key).eval()
    MG.fill(w.diffusion_model, 11)
    return w


def wrapper_cases(ddpm3d):
    T = SHAPE[0]
    out = {}
    w8 = wrapper_for(ddpm3d, dict(MG.REDUCED, in_channels=8), "hybrid")
    with torch.no_grad():
        x = MG.inp("hybrid.a.x", (1, 4) + SHAPE)
        ctx = MG.inp("hybrid.a.ctx", (1, 77, 128))
        cc0 = MG.inp("hybrid.a.cc0", (1, 4) + SHAPE)
        t = torch.tensor([500])
        scale = 1.0
        while True:                                   # the sensitivity condition (scales the c_concat INPUT only)
            a = w8(x, t, c_concat=[cc0 * scale], c_crossattn=[ctx])
            a_zero = w8(x, t, c_concat=[torch.zeros_like(cc0)], c_crossattn=[ctx])
            sens = relerr(a_zero, a)
            print(f"[hybrid] a: out std {a.std():.4f}; c_concat -> zeros moves it by {sens:.3e} of max|a| (need > {SENSITIVITY:.2e}), "
                  f"c_concat scale {scale}")
            if sens > SENSITIVITY:
                break
            scale *= 2.0
        out.update(a=a, a_zero=a_zero, a__t=t, concat_scale=np.asarray(scale))
        # d: fps in the call is dropped by the hybrid branch -- proven on the reference, not assumed
        d = w8(x, t, c_concat=[cc0 * scale], c_crossattn=[ctx], fps=torch.tensor([10]))
        assert torch.equal(d, a), "the reference's 'hybrid' branch forwarded fps"
        out.update(d=d, d__t=t, d__fps=np.asarray([10]))
        tb = torch.tensor([int(v) for v in np.linspace(999, 0, T).round()])
        out.update(b=w8(MG.inp("hybrid.b.x", (1, 4) + SHAPE), tb, c_concat=[MG.inp("hybrid.b.cc0", (1, 4) + SHAPE) * scale],
                        c_crossattn=[MG.inp("hybrid.b.ctx", (1, 77, 128))]), b__t=tb)
        tc = torch.tensor([981, 20])
        out.update(c=w8(MG.inp("hybrid.c.x", (2, 4) + SHAPE), tc,
                        c_concat=[MG.inp("hybrid.c.cc0", (2, 2) + SHAPE) * scale, MG.inp("hybrid.c.cc1", (2, 2) + SHAPE) * scale],
                        c_crossattn=[MG.inp("hybrid.c.ctx", (2, 77, 128))]), c__t=tc)
        w9 = wrapper_for(ddpm3d, dict(MG.REDUCED, in_channels=9), "hybrid-adm-mask")
        out.update(e=w9(MG.inp("hybrid.e.x", (1, 4) + SHAPE), t,
                        c_concat=[MG.inp("hybrid.e.cc0", (1, 4) + SHAPE) * scale, MG.inp("hybrid.e.cc1", (1, 1) + SHAPE) * scale],
                        c_crossattn=[MG.inp("hybrid.e.ctx", (1, 77, 128))], s=torch.tensor([3]), mask=torch.ones(1, 1, *SHAPE)),
                   e__t=t)
    for k in "abcde":
        print(f"[hybrid] {k}: {tuple(out[k].shape)} std {out[k].std():.4f}")
    MG.save("hybrid_wrapper", **out)
    return w8, scale


def sample_case(ddpm3d, w8, scale):
    """loop_base's settings (tools/make_golden.py::loop_cases) on the hybrid model: S = 10, eta 1, CFG 12, use_scale"""
    from lvdm.models.samplers import ddim as D
    D.DDIMSampler.register_buffer = lambda self, name, attr: setattr(self, name, attr)
    D.DDIMSampler.initialize_segmentation_models = lambda self: None

    class Model(MG.FakeModel):
        model = w8
        apply_model = ddpm3d.LatentDiffusion.apply_model

    model = Model()
    shape = (1, 4) + SHAPE
    x_T = MG.inp("hybrid.sample.x_T", shape)
    noises = [MG.inp(f"hybrid.sample.noise{i}", shape) for i in range(10)]
    q = list(noises)
    real = D.noise_like
    D.noise_like = lambda shp, dev, repeat=False: q.pop(0).clone()
    try:
        s = D.DDIMSampler(model)
        cc = [MG.inp("hybrid.sample.cc0", shape) * scale]
        cond = {"c_concat": cc, "c_crossattn": [MG.inp("hybrid.sample.ctx", (1, 77, 128))], "fps": torch.tensor([10])}
        uc = {k: cond[k] for k in cond}                                     # funcs.py:211-214
        uc.update({"c_crossattn": [MG.inp("hybrid.sample.uctx", (1, 77, 128))]})
        t0 = time.time()
        with torch.no_grad():
            samples, _ = s.sample(S=10, conditioning=cond, batch_size=1, shape=shape[1:], verbose=False,
                                  unconditional_guidance_scale=12.0, unconditional_conditioning=uc, eta=1.0, x_T=x_T)
    finally:
        D.noise_like = real
    assert not q, "the loop drew fewer noises than recorded"
    print(f"[hybrid] sample: {time.time() - t0:.1f}s, std {samples.std():.3f} max {samples.abs().max():.2f}")
    MG.save("hybrid_sample", samples=samples, concat_scale=np.asarray(scale))


def full_case(ddpm3d):
    import yaml
    with open(os.path.join(MG.REF, "configs/inference_t2v_512_v2.0.yaml")) as f:
        params = dict(yaml.safe_load(f)["model"]["params"]["unet_config"]["params"])
    params.update(use_checkpoint=False, in_channels=8)
    w = wrapper_for(ddpm3d, params, "hybrid")
    shp = (16, 40, 64)
    with torch.no_grad():
        t0 = time.time()
        y = w(MG.inp("full_hybrid.x", (1, 4) + shp), torch.tensor([500]), c_concat=[MG.inp("full_hybrid.cc0", (1, 4) + shp)],
              c_crossattn=[MG.inp("full_hybrid.ctx", (1, 77, 1024))])
    print(f"[full_hybrid] forward {time.time() - t0:.1f}s, out std {y.std():.4f}")
    MG.save("unet_full_hybrid", hybrid=y, hybrid__t=torch.tensor([500]), hybrid__L=np.asarray(77))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--full", action="store_true")
    ap.add_argument("--only-full", action="store_true")
    a = ap.parse_args()
    torch.set_num_threads(8)
    MG.import_reference()
    from lvdm.models import ddpm3d
    if not a.only_full:
        w8, scale = wrapper_cases(ddpm3d)
        sample_case(ddpm3d, w8, scale)
    if a.full or a.only_full:
        full_case(ddpm3d)


if __name__ == "__main__":
    main()
