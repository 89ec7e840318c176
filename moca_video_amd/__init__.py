"""moca_video_amd -- MI355X (gfx950) native denoising hot path of MoCA-Video / VideoCrafter2.

Public surface mirrors the reference interfaces for this path only:
  UNetModel            lvdm/modules/networks/openaimodel3d.py:279-578
  DiffusionWrapper     lvdm/models/ddpm3d.py:696-763
  DenoiseModel         the slice of LatentDiffusion the samplers use (apply_model + schedule buffers) and its own DDPM sampler:
                       q_sample, predict_start_from_noise, q_posterior, p_mean_variance, p_sample, p_sample_loop with masked
                       inpainting (ddpm3d.py:136-153,212-225,412-420,565-657; moca_video_amd.ddpm)
  DDIMSampler          lvdm/models/samplers/ddim.py (make_schedule, p_sample_ddim, unet, ddim_step, fifo_onestep,
                       stochastic_encode, decode, ddim_inversion; encode: deterministic DDIM inversion, upstream's third method)
  freq_mix_3d, get_freq_filter   utils/freeinit_utils.py
  prepare_latents, shift_latents, fifo_ddim_sampling, base_ddim_sampling   scripts/evaluation/funcs.py
  fifo_ddim_sampling_multiprompts   funcs.py:375-468 (one video, prompts switched inside the one-graph loop)
  v2v_ddim_sampling    DDIMSampler.stochastic_encode + decode (ddim.py:652-692): noise a clip's latents, denoise under a new prompt
  v2v_invert_sampling  DDIMSampler.encode + decode: the clip's own DDIM inversion in place of the noising, then denoise under a new prompt
  freeinit_ddim_sampling   FreeInit (Wu et al., 2023) over base_ddim_sampling: re-noise with the initial noise, freq_mix_3d, sample again
  DPMSolverSampler     DPM-Solver++(2M) (Lu et al., 2022) on DDIMSampler's timestep grid and one-graph step; no counterpart in the reference
  dpm_solver_sampling, v2v_dpm_solver_sampling   base_ddim_sampling / v2v_ddim_sampling with that solver (20 steps where DDIM takes 50)
  inpaint_ddim_sampling, inpaint_dpm_solver_sampling   masked inpainting (keep the clip where mask == 1) at DDIM / DPM-Solver speed:
                       upstream's blend in front of every step of the one-graph loop (DDIMSampler.sample / decode with mask=, x0=)
  load_multiprompts, run_multiprompts  its prompt file and driver (moca_video_amd.io)
  instantiate_from_config       utils/utils.py:27-42
  AutoencoderKL                 lvdm/models/autoencoder.py:13-107 + lvdm/modules/networks/ae_modules.py:364-579
  FrozenOpenCLIPEmbedder        lvdm/modules/encoders/condition.py:174-235 (text tower on token ids)
  SimpleTokenizer               what open_clip.tokenize does (condition.py:207): byte-level BPE, needs the CLIP merges file
  FrozenOpenCLIPImageEmbedderV2, FrozenOpenCLIPImageEmbedder   condition.py:298-376 / :238-296 (OpenCLIP ViT-H/14 vision tower)
  LatentVisualDiffusion         lvdm/models/ddpm3d.py:660-692 (image-conditioned model)
  Resampler, ImageProjModel     lvdm/modules/encoders/ip_resampler.py (image projectors)
Importing the package loads libmoca_hip.so and fails loudly if it has not been built.
"""
from . import lib as _lib

_lib.load()

from .unet import UNetModel  # noqa: E402
from .wrapper import DiffusionWrapper, DenoiseModel, instantiate_from_config, load_unet_config  # noqa: E402
from .vae import AutoencoderKL  # noqa: E402
from .clip_text import FrozenOpenCLIPEmbedder  # noqa: E402
from .tokenizer import SimpleTokenizer  # noqa: E402
from .image_proj import ImageProjModel, Resampler  # noqa: E402
from .clip_vision import FrozenOpenCLIPImageEmbedder, FrozenOpenCLIPImageEmbedderV2  # noqa: E402
from .wrapper import LatentVisualDiffusion  # noqa: E402
from .fifo import fifo_ddim_sampling_multiprompts, freeinit_ddim_sampling, v2v_ddim_sampling, v2v_invert_sampling  # noqa: E402
from .fifo import dpm_solver_sampling, v2v_dpm_solver_sampling  # noqa: E402
from .fifo import inpaint_ddim_sampling, inpaint_dpm_solver_sampling  # noqa: E402
from .sampler import DPMSolverSampler  # noqa: E402
from .io import load_multiprompts, run_multiprompts  # noqa: E402

__all__ = ["UNetModel", "DiffusionWrapper", "DenoiseModel", "AutoencoderKL", "FrozenOpenCLIPEmbedder", "SimpleTokenizer", "ImageProjModel", "Resampler",
           "FrozenOpenCLIPImageEmbedder", "FrozenOpenCLIPImageEmbedderV2", "LatentVisualDiffusion", "instantiate_from_config",
           "load_unet_config", "fifo_ddim_sampling_multiprompts", "v2v_ddim_sampling", "v2v_invert_sampling", "freeinit_ddim_sampling", "load_multiprompts", "run_multiprompts",
           "DPMSolverSampler", "dpm_solver_sampling", "v2v_dpm_solver_sampling",
           "inpaint_ddim_sampling", "inpaint_dpm_solver_sampling"]
