"""Shared pieces of the video-to-video tests (tests/test_v2v_cpu.py, tests/test_v2v_gpu.py): the reference's signatures, a model that
holds only what `DDIMSampler.make_schedule` reads, and the stub first stage of the `ddim_inversion` goldens
(tools/make_golden_v2v.py::inversion_case)."""
from functools import partial

import numpy as np
import torch

# lvdm/models/samplers/ddim.py:652, :674-675, :972 -- parameter names after `self`, in order
REF_SIGNATURES = {
    "stochastic_encode": ["x0", "t", "use_original_steps", "noise"],
    "decode": ["x_latent", "cond", "t_start", "unconditional_guidance_scale", "unconditional_conditioning", "use_original_steps"],
    "ddim_inversion": ["frames", "num_inference_steps", "eta", "latents_dir"],
}
S, T_START, SCALE = 10, 6, 12.0
SHAPE = (1, 4, 8, 16, 16)


class ScheduleModel:
    """the DDPM buffers of `LatentDiffusion.register_schedule` (ddpm3d.py:113-165,362-376) and nothing else"""

    def __init__(self, device="cpu"):
        from moca_video_amd.wrapper import make_beta_schedule
        betas = make_beta_schedule("linear", 1000, linear_start=0.00085, linear_end=0.012)
        ac = np.cumprod(1. - betas, axis=0)
        to_torch = partial(torch.tensor, dtype=torch.float32, device=device)
        self.num_timesteps = 1000
        self.betas = to_torch(betas)
        self.alphas_cumprod = to_torch(ac)
        self.alphas_cumprod_prev = to_torch(np.append(1., ac[:-1]))
        self.use_scale = True
        self.scale_arr = to_torch(np.concatenate((np.linspace(1, 0.7, 400), np.full(1000, 0.7))))
        self.device = torch.device(device)


class StubFirstStage(ScheduleModel):
    """`encode_first_stage_2DAE` returns a fixed z and records the shape it was shown"""

    def __init__(self, z, device="cuda"):
        super().__init__(device)
        self.z, self.seen = z, None

    def encode_first_stage_2DAE(self, frames, noise=None):
        self.seen = tuple(frames.shape)
        return self.z.clone()
