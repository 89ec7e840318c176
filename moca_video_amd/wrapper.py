"""Drop-in boundary above the UNet: `DiffusionWrapper.forward` (lvdm/models/ddpm3d.py:702-763,
`crossattn` branch :710-712 and the `hybrid*` branches :713-759) and the slice of `LatentDiffusion` the samplers touch:
`apply_model` (:512-527), the DDPM schedule buffers (`register_schedule`, :113-165) and
`scale_arr` (:362-376).  VAE / text encoder / training scaffolding are out of scope."""
from __future__ import annotations

import importlib
from functools import partial

import numpy as np
import torch
import torch.nn as nn

from .conditioning import CONTEXT_FREE_KEYS, HYBRID_KEYS  # noqa: F401  (re-exported: the keys DiffusionWrapper.forward branches on)
from .ddpm import DdpmMixin
from .unet import UNetModel

# `target:` strings of the reference YAML resolve to our classes, so an unmodified
# configs/inference_t2v_512_v2.0.yaml instantiates the MI355X path.
def _vae_cls(**kw):
    from .vae import AutoencoderKL
    return AutoencoderKL(**kw)


_TARGET_ALIASES = {
    "lvdm.modules.networks.openaimodel3d.UNetModel": UNetModel,
    "lvdm.models.autoencoder.AutoencoderKL": _vae_cls,
    "lvdm.modules.encoders.condition.FrozenOpenCLIPEmbedder": lambda **kw: _clip_cls(**kw),
}


def _clip_cls(**kw):
    from .clip_text import FrozenOpenCLIPEmbedder
    return FrozenOpenCLIPEmbedder(**kw)


def get_obj_from_str(string):
    if string in _TARGET_ALIASES:
        return _TARGET_ALIASES[string]
    module, cls = string.rsplit(".", 1)
    return getattr(importlib.import_module(module, package=None), cls)


def instantiate_from_config(config):
    """utils/utils.py:27-34"""
    if "target" not in config:
        if config == '__is_first_stage__':
            return None
        elif config == "__is_unconditional__":
            return None
        raise KeyError("Expected key `target` to instantiate.")
    return get_obj_from_str(config["target"])(**config.get("params", dict()))


def load_unet_config(yaml_path):
    """unet_config block of configs/inference_t2v_512_v2.0.yaml (:22-50) as a plain dict."""
    import yaml
    with open(yaml_path) as f:
        cfg = yaml.safe_load(f)
    return cfg["model"]["params"]["unet_config"], cfg["model"]["params"]


class DiffusionWrapper(nn.Module):
    """lvdm/models/ddpm3d.py:696-763: `crossattn` and the five `hybrid*` keys (x and the `c_concat` latents concatenated along the
    channel axis, `c_crossattn` as the context).  The hybrid branches keep the reference's argument handling: `**kwargs` (so a
    `fps` of the conditioning dict) are NOT forwarded and the UNet runs with its default fps=16; `y=` / `s=` / `mask=` are passed
    and ignored by the UNet as upstream.  The concat is not materialised for our UNet (`UNetModel.forward_concat`).
    `features_adapter=` (openaimodel3d.py:562-567) rides in `**kwargs`: `crossattn` hands it to the UNet, the hybrid keys refuse it."""

    def __init__(self, diff_model_config, conditioning_key):
        super().__init__()
        self.diffusion_model = instantiate_from_config(diff_model_config)
        self.conditioning_key = conditioning_key

    def forward(self, x, t, c_concat: list = None, c_crossattn: list = None, c_adm=None, s=None, mask=None, **kwargs):
        if self.conditioning_key in HYBRID_KEYS and kwargs.get("features_adapter") is not None:
            # (upstream drops **kwargs on these branches, so the maps would silently not be applied: refused instead)
            raise NotImplementedError(f"features_adapter with conditioning_key={self.conditioning_key!r}: the adapter maps reach the UNet "
                                      "through the 'crossattn' key only")
        if self.conditioning_key == 'crossattn':
            cc = torch.cat(c_crossattn, 1)                                   # :711
            out = self.diffusion_model(x, t, context=cc, **kwargs)           # :712
        elif self.conditioning_key == 'hybrid':
            out = self._hybrid(x, t, c_concat, c_crossattn)                  # :715-717 (no **kwargs: fps is dropped)
        elif self.conditioning_key == 'hybrid-adm':
            assert c_adm is not None                                         # :725
            out = self._hybrid(x, t, c_concat, c_crossattn, y=c_adm)
        elif self.conditioning_key == 'hybrid-time':
            assert s is not None                                             # :730
            out = self._hybrid(x, t, c_concat, c_crossattn, s=s)
        elif self.conditioning_key == 'hybrid-adm-mask':
            out = self._hybrid(x, t, c_concat, c_crossattn, concat_optional=True, y=s, mask=mask)     # :748-753
        elif self.conditioning_key == 'hybrid-time-adm':
            assert c_adm is not None                                         # :756
            out = self._hybrid(x, t, c_concat, c_crossattn, s=s, y=c_adm)
        elif self.conditioning_key in CONTEXT_FREE_KEYS:
            raise NotImplementedError(f"conditioning_key={self.conditioning_key!r} calls the UNet without a context, which the reference's "
                                      "own UNet cannot run either (openaimodel3d.py:547: context.repeat_interleave on None)")
        else:
            raise NotImplementedError(f"conditioning_key={self.conditioning_key!r}")
        return out

    def _hybrid(self, x, t, c_concat, c_crossattn, concat_optional=False, **unet_kwargs):
        """`xc = torch.cat([x] + c_concat, dim=1); diffusion_model(xc, t, context=cat(c_crossattn, 1), **unet_kwargs)`"""
        cc = torch.cat(c_crossattn, 1)
        if c_concat is None and concat_optional:
            pieces = []                                                      # :749-752 (`xc = x`)
        else:
            if c_concat is None:
                raise TypeError("c_concat is None (upstream: `[x] + c_concat`); only 'hybrid-adm-mask' runs without it")
            pieces = list(c_concat)
        want = getattr(self.diffusion_model, "in_channels", None)
        total = x.shape[1] + sum(int(p.shape[1]) for p in pieces)
        if want is not None and total != want:
            raise ValueError(f"conditioning_key={self.conditioning_key!r}: x has {x.shape[1]} channels and c_concat "
                             f"{[int(p.shape[1]) for p in pieces]}, {total} in all; the UNet was built with in_channels={want}")
        if not pieces:
            return self.diffusion_model(x, t, context=cc, **unet_kwargs)
        if hasattr(self.diffusion_model, "forward_concat"):                  # our UNet: the pieces go straight into the first conv's rows
            return self.diffusion_model.forward_concat(x, pieces, t, context=cc, **unet_kwargs)
        return self.diffusion_model(torch.cat([x] + pieces, dim=1), t, context=cc, **unet_kwargs)


def make_beta_schedule(schedule, n_timestep, linear_start=1e-4, linear_end=2e-2):
    """utils_diffusion.py:31-53 (the 'linear' branch the YAML uses)"""
    if schedule != "linear":
        raise NotImplementedError(schedule)
    betas = torch.linspace(linear_start ** 0.5, linear_end ** 0.5, n_timestep, dtype=torch.float64, device="cpu") ** 2
    return betas.numpy()


class DenoiseModel(DdpmMixin, nn.Module):
    """What `DDIMSampler` needs from `LatentDiffusion`: `apply_model`, `num_timesteps`, `betas`,
    `alphas_cumprod(_prev)`, `use_scale`/`scale_arr`, `device` (ddpm3d.py:83-165,362-376,512-527); and the model's own DDPM
    sampler -- posterior tables, `q_sample`, `p_sample`, `p_sample_loop` with masked inpainting -- from `ddpm.DdpmMixin`."""

    def __init__(self, unet_config, timesteps=1000, linear_start=0.00085, linear_end=0.012, conditioning_key="crossattn",
                 use_scale=True, scale_a=1, scale_b=0.7, mid_step=400, fix_scale_bug=False, parameterization="eps",
                 uncond_type="empty_seq", first_stage_config=None, scale_factor=1.0, cond_stage_config=None, v_posterior=0.,
                 log_every_t=100, **ignored):
        super().__init__()
        self.parameterization = parameterization
        self.v_posterior = v_posterior                   # ddpm3d.py:93: weight of the posterior variance, sigma = (1-v) beta_tilde + v beta
        self.log_every_t = log_every_t                   # :75
        self.clip_denoised = False                       # :390 (LatentDiffusion: what p_sample_loop hands to p_sample)
        self.uncond_type = uncond_type
        self.model = DiffusionWrapper(unet_config, conditioning_key)
        self.num_timesteps = int(timesteps)
        # register_schedule, ddpm3d.py:113-165
        betas = make_beta_schedule("linear", timesteps, linear_start=linear_start, linear_end=linear_end)
        self._betas64 = betas                            # float64: the posterior tables (ddpm.ddpm_tables) are derived from these
        alphas = 1. - betas
        alphas_cumprod = np.cumprod(alphas, axis=0)
        alphas_cumprod_prev = np.append(1., alphas_cumprod[:-1])
        to_torch = partial(torch.tensor, dtype=torch.float32)
        self.register_buffer('betas', to_torch(betas))
        self.register_buffer('alphas_cumprod', to_torch(alphas_cumprod))
        self.register_buffer('alphas_cumprod_prev', to_torch(alphas_cumprod_prev))
        self.register_buffer('sqrt_alphas_cumprod', to_torch(np.sqrt(alphas_cumprod)))
        self.register_buffer('sqrt_one_minus_alphas_cumprod', to_torch(np.sqrt(1. - alphas_cumprod)))
        # scale_arr, ddpm3d.py:362-376 (the "bug" branch: length mid_step + num_timesteps = 1400)
        self.use_scale = use_scale
        if use_scale:
            scale_step = self.num_timesteps - mid_step if fix_scale_bug else self.num_timesteps
            scale_arr = np.concatenate((np.linspace(scale_a, scale_b, mid_step), np.full(scale_step, scale_b)))
            self.register_buffer('scale_arr', to_torch(scale_arr))
        # first stage (ddpm3d.py:383,386,431-437): only the decode side is on the MoCA path (funcs.py:360)
        self.scale_factor = scale_factor
        self.first_stage_model = instantiate_from_config(first_stage_config) if first_stage_config is not None else None
        self.cond_stage_model = instantiate_from_config(cond_stage_config) if cond_stage_config is not None else None

    def get_learned_conditioning(self, c):
        """ddpm3d.py:440-455 (cond_stage_forward is None: `self.cond_stage_model.encode(c)`); `c` = token ids [B, 77] -- the BPE
        tokenizer of open_clip is the caller's (not available offline)"""
        if self.cond_stage_model is None:
            raise RuntimeError("DenoiseModel was built without cond_stage_config")
        return self.cond_stage_model.encode(c)

    @torch.no_grad()
    def decode_first_stage_2DAE(self, z, **kwargs):
        """ddpm3d.py:556-562: z [b,c,t,h,w] latents -> [b,3,t,8h,8w]; the reference decodes one frame per call, here
        all b*t frames go through the recorded decoder in groups of `AutoencoderKL.max_frames_per_launch`."""
        if self.first_stage_model is None:
            raise RuntimeError("DenoiseModel was built without first_stage_config")
        b, c, t, h, w = z.shape
        zf = (1. / self.scale_factor * z).permute(0, 2, 1, 3, 4).reshape(b * t, c, h, w)
        out = self.first_stage_model.decode(zf, **kwargs)
        return out.reshape(b, t, *out.shape[1:]).permute(0, 2, 1, 3, 4).contiguous()

    def get_first_stage_encoding(self, encoder_posterior, noise=None):
        """ddpm3d.py:458-465"""
        from .vae import DiagonalGaussianDistribution
        if isinstance(encoder_posterior, DiagonalGaussianDistribution):
            z = encoder_posterior.sample(noise=noise)
        elif isinstance(encoder_posterior, torch.Tensor):
            z = encoder_posterior
        else:
            raise NotImplementedError(f"encoder_posterior of type '{type(encoder_posterior)}' not yet implemented")
        return self.scale_factor * z

    @torch.no_grad()
    def encode_first_stage_2DAE(self, x, noise=None):
        """ddpm3d.py:496-502: x [b,3,t,H,W] -> latents [b,4,t,H/8,W/8]; the reference encodes (and samples) frame by
        frame, here all frames go through the recorded encoder together (`noise` [b,4,t,h,w] optionally fixes the draw)."""
        if self.first_stage_model is None:
            raise RuntimeError("DenoiseModel was built without first_stage_config")
        b, c, t, H, W = x.shape
        post = self.first_stage_model.encode(x.permute(0, 2, 1, 3, 4).reshape(b * t, c, H, W))
        if noise is not None:
            noise = noise.permute(0, 2, 1, 3, 4).reshape(b * t, *noise.shape[1:2], *noise.shape[3:])
        z = self.get_first_stage_encoding(post, noise=noise)
        return z.reshape(b, t, *z.shape[1:]).permute(0, 2, 1, 3, 4).contiguous()

    @property
    def device(self):
        return self.betas.device

    def apply_model(self, x_noisy, t, cond, **kwargs):
        """ddpm3d.py:512-527"""
        if isinstance(cond, dict):
            pass
        else:
            if not isinstance(cond, list):
                cond = [cond]
            key = 'c_concat' if self.model.conditioning_key == 'concat' else 'c_crossattn'
            cond = {key: cond}
        x_recon = self.model(x_noisy, t, **cond, **kwargs)
        if isinstance(x_recon, tuple):
            return x_recon[0]
        return x_recon


class LatentVisualDiffusion(DenoiseModel):
    """ddpm3d.py:660-692: the image-conditioned model of the i2v configs.  `image_proj_model` is the HIP projector the reference's
    `init_projector` picks (`Resampler` with 16 queries for `finegrained`, else `ImageProjModel` with 4 tokens; output dim 1024, so the UNet
    needs `context_dim: 1024`).  The image embedder (the OpenCLIP ViT-H/14 vision tower, condition.py:298-376) is instantiated from
    `cond_img_config` when that target imports -- `moca_video_amd.clip_vision.FrozenOpenCLIPImageEmbedderV2` (or
    `FrozenOpenCLIPImageEmbedder`) is the HIP one -- otherwise it stays None and the caller assigns `.embedder`; `get_image_embeds`
    raises without one.  `project_image_features` runs the projector on precomputed features
    ([B, 257, 1280] for the Resampler, [B, 1024] for ImageProjModel)."""

    def __init__(self, cond_img_config=None, finegrained=False, random_cond=False, *args, **kwargs):
        super().__init__(*args, **kwargs)
        from .image_proj import ImageProjModel, Resampler
        self.random_cond = random_cond
        self.finegrained = finegrained
        self.embedder = None
        if cond_img_config is not None:
            try:
                get_obj_from_str(cond_img_config["target"])
            except (ImportError, AttributeError):
                pass                                     # the seam: the caller assigns .embedder
            else:
                self.embedder = instantiate_from_config(cond_img_config).eval()
                for p in self.embedder.parameters():
                    p.requires_grad = False
        num_tokens = 16 if finegrained else 4
        if finegrained:
            self.image_proj_model = Resampler(dim=1024, depth=4, dim_head=64, heads=12, num_queries=num_tokens, embedding_dim=1280,
                                              output_dim=1024, ff_mult=4)
        else:
            self.image_proj_model = ImageProjModel(clip_extra_context_tokens=num_tokens, cross_attention_dim=1024, clip_embeddings_dim=1024)

    def project_image_features(self, feats):
        """the projector on precomputed image features"""
        return self.image_proj_model(feats)

    @torch.no_grad()
    def get_image_embeds(self, batch_imgs):
        """ddpm3d.py:689-693: img [b, c, h, w] -> image tokens [b, 16 | 4, 1024]"""
        if self.embedder is None:
            raise RuntimeError("LatentVisualDiffusion has no image embedder: cond_img_config's target did not import (the HIP vision tower "
                               "is moca_video_amd.clip_vision.FrozenOpenCLIPImageEmbedderV2); assign `.embedder` or call "
                               "project_image_features on features")
        return self.image_proj_model(self.embedder(batch_imgs))
