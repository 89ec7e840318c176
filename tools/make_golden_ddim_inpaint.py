#!/usr/bin/env python3
"""Generate the DDIM-inpainting goldens by running the REAL reference on the CPU: the real reduced-width UNet inside the real
`DiffusionWrapper` through the real `LatentDiffusion.apply_model`, the real `DDIMSampler.make_schedule` and `p_sample_ddim`
(lvdm/models/samplers/ddim.py:62-106, :274-359) and the real `LatentDiffusion.q_sample` (lvdm/models/ddpm3d.py:412-420).  The
reference's `ddim_sampling` declares `mask` / `x0` and never reads the mask; the loop here is its loop (:232-247) with the two lines of
the upstream latent-diffusion sampler it derives from put back, in upstream's order -- before the model call of every step:

    img_orig = model.q_sample(x0, ts)
    img = img_orig * mask + (1. - mask) * img

  ddim_inpaint.npz         loop_base's settings (shape [1,4,8,16,16], S = 10, eta 1, guidance 12, use_scale, loop_base's contexts, fps
                           10), named x_T / x0 / step noises / q-noises (tests/ddim_inpaint_ref.py): a = one-channel spatial mask
                           [1,1,1,16,16], left half kept; b = frame mask keeping frames 0-2 (read as "full"); c = `decode` from
                           t_start = 6 (x0 noised by the real `stochastic_encode`) with mask a; d = mask a at eta 0 without use_scale.
                           Per case the final latents and the sensitivities below; for c also x_enc.
  ddim_inpaint_eps_<case>.npz   the guided model output e_t of every step of that case (ddim.py:304), recorded from the real run: with
                           them the fp32 torch restatement of the loop (tests/ddim_inpaint_ref.py) reproduces the case EXACTLY on a CPU.

Fixture sensitivity, measured with the reference itself and ASSERTED here, per case: dropping the blend, taking q_sample at the
neighbouring schedule row, and blending after the step instead of before it (the DDPM loop's order) must each move the result by more
than 3 x TOL_BASE of max|ref|.

    python tools/make_golden_ddim_inpaint.py

The fp32 square roots `p_sample_ddim` and `stochastic_encode` take are pinned to the correctly rounded result (`pinned_sqrt`, here also
for `Tensor.sqrt`), so that the exact goldens do not depend on the CPU the tool ran on.  Same recipe as tools/make_golden.py (whose
helpers it imports): parameters and inputs are regenerated bit-identically from moca_video_amd.weightgen by name, so a fixture holds
only the expected outputs and the call metadata."""
import contextlib
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as MG  # noqa: E402
import make_golden_v2v as V2V  # noqa: E402  (puts tests/ on the path)

from ddim_inpaint_ref import CASES, S, SCALE, SHAPE, T_START, conds, mask_of, operands  # noqa: E402
from test_loops_gpu import TOL_BASE  # noqa: E402

FACTOR = 3.0                      # sensitivity margin over TOL_BASE


@contextlib.contextmanager
def pinned_sqrt():
    """`make_golden_v2v.pinned_sqrt`, extended to the method form `t.sqrt()` that p_sample_ddim uses (ddim.py:339,343,355)"""
    real = torch.Tensor.sqrt
    with V2V.pinned_sqrt() as changed:
        torch.Tensor.sqrt = lambda self: torch.sqrt(self)
        try:
            yield changed
        finally:
            torch.Tensor.sqrt = real


def build_model(ddpm3d):
    from lvdm.models.utils_diffusion import make_beta_schedule
    wrapper = ddpm3d.DiffusionWrapper({"target": "lvdm.modules.networks.openaimodel3d.UNetModel", "params": dict(MG.REDUCED)},
                                      "crossattn").eval()
    MG.fill(wrapper.diffusion_model, 11)

    class Model(MG.FakeModel):
        model = wrapper
        apply_model = ddpm3d.LatentDiffusion.apply_model
        q_sample = ddpm3d.LatentDiffusion.q_sample

        def __init__(self):
            super().__init__()
            ac = np.cumprod(1. - make_beta_schedule("linear", 1000, linear_start=0.00085, linear_end=0.012), axis=0)
            self.sqrt_alphas_cumprod = torch.tensor(np.sqrt(ac), dtype=torch.float32)                  # ddpm3d.py:137-138
            self.sqrt_one_minus_alphas_cumprod = torch.tensor(np.sqrt(1. - ac), dtype=torch.float32)

    return Model()


def run_case(D, model, case):
    mask_name, eta, use_scale, n_rows = CASES[case]
    model.use_scale = use_scale
    cond, uc = conds()
    o = operands(case)
    mask, x0 = mask_of(mask_name), o["x0"]
    s = D.DDIMSampler(model)
    with V2V.quiet():
        s.make_schedule(S, ddim_eta=eta, verbose=False)
    with torch.no_grad(), pinned_sqrt():
        x_start = o["x_T"] if n_rows == S else s.stochastic_encode(x0, torch.tensor([n_rows]), noise=o["enc_noise"])
    real_noise_like, real_apply = D.noise_like, model.apply_model

    def loop(blend="before", q_row_shift=0, record=None):
        q = list(o["noises"])
        D.noise_like = lambda shp, dev, repeat=False: q.pop(0).clone()
        outs = []
        if record is not None:
            model.apply_model = lambda x, t, c, **kw: outs.append(real_apply(x, t, c, **kw)) or outs[-1]
        img = x_start

        def blended(img, i, index):
            r = index + q_row_shift
            r = r if r < S else index - q_row_shift                         # (the neighbour below where there is none above)
            tq = torch.full((SHAPE[0],), int(s.ddim_timesteps[r]), dtype=torch.long)
            img_orig = model.q_sample(x0, tq, noise=o["mask_noises"][i])
            return img_orig * mask + (1. - mask) * img
        try:
            with torch.no_grad(), pinned_sqrt():
                for i, step in enumerate(np.flip(s.ddim_timesteps[:n_rows])):        # ddim.py:223,232-247
                    index = n_rows - i - 1
                    ts = torch.full((SHAPE[0],), int(step), dtype=torch.long)
                    if blend == "before":
                        img = blended(img, i, index)
                    img, _ = s.p_sample_ddim(img, cond, ts, index=index, unconditional_guidance_scale=SCALE, unconditional_conditioning=uc)
                    if blend == "after":
                        img = blended(img, i, index)
                    if record is not None:                                           # e_t = e_u + s (e_c - e_u), :304, the same torch ops
                        e_c, e_u = outs
                        record.append(e_u + SCALE * (e_c - e_u))
                        del outs[:]
        finally:
            D.noise_like = real_noise_like
            if record is not None:
                del model.apply_model
        assert not q, "the loop drew another number of noises than steps"
        return img

    t0 = time.time()
    eps = []
    ref = loop(record=eps)
    print(f"[inpaint] case {case}: {n_rows} steps {time.time() - t0:.1f}s, std {ref.std():.3f} max {ref.abs().max():.2f}")
    need = FACTOR * TOL_BASE
    moved = {"no blend": V2V.relerr(loop(blend=None), ref), "q_sample at the neighbouring row": V2V.relerr(loop(q_row_shift=1), ref),
             "blend after the step": V2V.relerr(loop(blend="after"), ref)}
    for k, v in moved.items():
        print(f"[inpaint] case {case} sensitivity, {k}: the result moves by {v:.3e} of max|ref| (need > {need:.2e}, margin {v / need:.1f} x)")
    assert all(v > need for v in moved.values()), "the fixture does not separate these from TOL_BASE: scale x0 or enlarge the kept area"
    MG.save(f"ddim_inpaint_eps_{case}", eps=torch.stack(eps))
    out = {case: ref, case + "__sens": np.asarray(list(moved.values()))}
    if n_rows != S:
        out[case + "__x_enc"] = x_start                                                  # an output too: the real stochastic_encode's
    return out


def main():
    torch.set_num_threads(16)
    MG.import_reference()
    from lvdm.models import ddpm3d
    D = V2V.patched_sampler_module()
    model = build_model(ddpm3d)
    out = {}
    for case in CASES:
        out.update(run_case(D, model, case))
    MG.save("ddim_inpaint", S=np.asarray(S), scale=np.asarray(SCALE), t_start=np.asarray(T_START), **out)


if __name__ == "__main__":
    main()
