"""The model class's own sampler: the DDPM side of `LatentDiffusion` (lvdm/models/ddpm3d.py) -- the posterior tables of
`register_schedule` (:136-153), `q_sample` (:412-420), `predict_start_from_noise` (:212-216), `q_posterior` (:218-225),
`p_mean_variance` (:565-588), `p_sample` (:591-610) and `p_sample_loop` (:613-657, the one place where the reference implements masked
inpainting: keep `x0` where `mask == 1`, regenerate the rest).  `DenoiseModel` inherits these from `DdpmMixin`.

All per-element arithmetic is ONE fp32 HIP kernel, `moca_ddpm_step_f32` (csrc/sampler.hip), in the reference's order of operations;
the host keeps the O(timesteps) table math (float64 numpy rounded once to fp32, as the reference's `to_torch`).  There is no CPU path.

The tables are NOT registered as buffers: they are derived from `betas` alone, and a `state_dict` that grew seven keys would change what
`load_state_dict(strict=True)` and whole-model weight fills see.  They are built lazily, cached per device, and read through attributes
of the reference's names (`model.posterior_variance` ...).

Extensions over the reference, all off by default: `noise=` / `noises=` / `mask_noises=` fix the draws (fixtures);
`unconditional_guidance_scale` / `unconditional_conditioning` apply classifier-free guidance by the formula of ddim.py:304 (the
reference's DDPM loop has none); `use_graph` picks the one-graph step (`fifo_graph.DdpmEngine`) or the host-issued loop."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import lib as _l
from . import ops
from .conditioning import _f32c, as_cond_dict, check_schedule_index, conditioning_key, guidance_eps
from .fifo_graph import DdpmEngine, EngineCache, mask_kind, mask_operand  # noqa: F401  (mask_kind, mask_operand: re-exported)

TABLE_NAMES = ("sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "log_one_minus_alphas_cumprod", "posterior_variance",
               "posterior_log_variance_clipped", "posterior_mean_coef1", "posterior_mean_coef2")


def ddpm_tables(betas, v_posterior=0.):
    """register_schedule, ddpm3d.py:120-153: float64 `betas` [n] -> the seven tables as fp32 numpy arrays (float64 math, rounded once)"""
    betas = np.asarray(betas, dtype=np.float64)
    alphas = 1. - betas
    alphas_cumprod = np.cumprod(alphas, axis=0)
    alphas_cumprod_prev = np.append(1., alphas_cumprod[:-1])
    posterior_variance = (1 - v_posterior) * betas * (1. - alphas_cumprod_prev) / (1. - alphas_cumprod) + v_posterior * betas
    t64 = {
        "sqrt_recip_alphas_cumprod": np.sqrt(1. / alphas_cumprod),
        "sqrt_recipm1_alphas_cumprod": np.sqrt(1. / alphas_cumprod - 1),
        "log_one_minus_alphas_cumprod": np.log(1. - alphas_cumprod),
        "posterior_variance": posterior_variance,
        "posterior_log_variance_clipped": np.log(np.maximum(posterior_variance, 1e-20)),
        "posterior_mean_coef1": betas * np.sqrt(alphas_cumprod_prev) / (1. - alphas_cumprod),
        "posterior_mean_coef2": (1. - alphas_cumprod_prev) * np.sqrt(alphas) / (1. - alphas_cumprod),
    }
    return {k: v.astype(np.float32) for k, v in t64.items()}


def ddpm_coef(tables, sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod, scale_arr=None):
    """the kernel's table coef[n][8] = {srac, srm1, c1, c2, std, sac, s1mac, scale} from fp32 tables.  std = exp(0.5 *
    posterior_log_variance_clipped) (:608, `(0.5 * model_log_variance).exp()`): the fp32 product is exact, the exponential is taken in
    float64 and rounded once, so no transcendental runs on the device and the value does not depend on the host's fp32 exp."""
    n = tables["posterior_variance"].shape[0]
    coef = np.ones((n, 8), np.float32)
    coef[:, 0] = tables["sqrt_recip_alphas_cumprod"]
    coef[:, 1] = tables["sqrt_recipm1_alphas_cumprod"]
    coef[:, 2] = tables["posterior_mean_coef1"]
    coef[:, 3] = tables["posterior_mean_coef2"]
    half_lv = np.float32(0.5) * tables["posterior_log_variance_clipped"]
    coef[:, 4] = np.exp(half_lv.astype(np.float64)).astype(np.float32)
    coef[:, 5] = np.asarray(sqrt_alphas_cumprod, np.float32)
    coef[:, 6] = np.asarray(sqrt_one_minus_alphas_cumprod, np.float32)
    if scale_arr is not None:
        coef[:, 7] = np.asarray(scale_arr, np.float32)[:n]
    return coef


def launch_ddpm_step(coef, t, *, B, per, x=None, out=None, eps_c=None, eps_u=None, noise=None, x_recon=None, mean=None, mask=None,
                     x0=None, noise_q=None, mask_inner=0, cfg_scale=1.0, temperature=1.0, flags=0, state=None, t_stride=1, stream=None):
    """`moca_ddpm_step_f32` on tensors (None = NULL); raises on a refused call"""
    p = _l.ptr
    st = C.c_void_p(ops.current_stream() if stream is None else stream)
    _l.check(_l.load().moca_ddpm_step_f32(p(state), p(x), p(out), p(eps_c), p(eps_u), p(noise), p(x_recon), p(mean), p(mask), p(x0),
                                          p(noise_q), p(coef), p(t), int(t_stride), int(B), int(coef.shape[0]), int(per),
                                          int(mask_inner), float(cfg_scale), float(temperature), int(flags), st), "moca_ddpm_step_f32")


engine_key = DdpmEngine.key          # (the name the key had when it lived here)


def _table_property(name):
    def get(self):
        return self._ddpm_dev(self.betas.device)[name]
    get.__doc__ = f"`{name}` of register_schedule (ddpm3d.py:136-153), fp32 [num_timesteps], on the model's device"
    return property(get)


class DdpmMixin:
    """the DDPM sampler surface of `LatentDiffusion`; the host class provides `betas` (buffer) and `_betas64`, `v_posterior`,
    `sqrt_alphas_cumprod`, `sqrt_one_minus_alphas_cumprod`, `use_scale` / `scale_arr`, `parameterization`, `apply_model`,
    `num_timesteps`, `log_every_t`, `clip_denoised`."""

    _ddpm_host_tables = None
    _ddpm_dev_tables = None

    @property
    def _ddpm_engines(self):
        """the cached step graph of `p_sample_loop` (made on first use: the mixin has no constructor)"""
        return self.__dict__.setdefault("_ddpm_engine_cache", EngineCache())

    _ddpm_engine = property(lambda self: self._ddpm_engines.entry, doc="None, or the (key, engine) of the cached step graph")

    def _ddpm_host(self):
        tabs = self._ddpm_host_tables
        if tabs is None:
            tabs = ddpm_tables(self._betas64, self.v_posterior)
            tabs["coef"] = ddpm_coef(tabs, self.sqrt_alphas_cumprod.detach().cpu().numpy(),
                                     self.sqrt_one_minus_alphas_cumprod.detach().cpu().numpy(),
                                     self.scale_arr.detach().cpu().numpy() if self.use_scale else None)
            self._ddpm_host_tables = tabs
        return tabs

    def _ddpm_dev(self, device):
        """the tables (and the kernel's packed `coef`) on `device`, built once per device"""
        if self._ddpm_dev_tables is None:
            self._ddpm_dev_tables = {}
        cache = self._ddpm_dev_tables
        key = str(torch.device(device))
        if key not in cache:
            cache[key] = {k: torch.from_numpy(v).to(device) for k, v in self._ddpm_host().items()}
        return cache[key]

    # ---- helpers ---------------------------------------------------------------------------------------------------------------
    def _ddpm_flags(self, clip=False, x0_param=None):
        x0p = (self.parameterization == "x0") if x0_param is None else x0_param
        if x0_param is None and self.parameterization not in ("eps", "x0"):
            raise NotImplementedError()                                          # :577-578
        return (_l.MOCA_DDPM_X0 if x0p else 0) | (_l.MOCA_DDPM_CLIP if clip else 0) | (_l.MOCA_DDPM_SCALE if self.use_scale else 0)

    def _ddpm_t(self, t, x):
        """per-sample timesteps as the kernel reads them: int64 [B] on x's device.  A host tensor is range-checked here (IndexError, as
        `extract_into_tensor`'s gather); a device tensor is gathered by the kernel (a t out of range gives that sample NaN)."""
        if not x.is_cuda:
            raise ValueError("the DDPM sampler runs on the GPU: the latents must be cuda tensors")
        return check_schedule_index(t, x.shape[0], self.num_timesteps, "timestep").to(x.device, torch.int64).contiguous()

    def _extract(self, name, t, x):
        return self._ddpm_dev(x.device)[name][t].reshape(x.shape[0], *((1,) * (x.dim() - 1)))    # extract_into_tensor, utils_diffusion.py

    # ---- the per-step methods --------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def q_sample(self, x_start, t, noise=None):
        """ddpm3d.py:412-420: sqrt_alphas_cumprod[t] x_start [scale_arr[t]] + sqrt_one_minus_alphas_cumprod[t] noise"""
        x_start = _f32c(x_start)
        t = self._ddpm_t(t, x_start)
        noise = torch.randn_like(x_start) if noise is None else _f32c(noise.to(x_start.device))
        if noise.shape != x_start.shape:
            raise ValueError(f"noise {tuple(noise.shape)} does not match x_start {tuple(x_start.shape)}")
        out = torch.empty_like(x_start)
        B = x_start.shape[0]
        launch_ddpm_step(self._ddpm_dev(x_start.device)["coef"], t, B=B, per=x_start.numel() // B, out=out, x0=x_start, noise_q=noise,
                         flags=self._ddpm_flags(x0_param=False))
        return out

    @torch.no_grad()
    def predict_start_from_noise(self, x_t, t, noise):
        """ddpm3d.py:212-216"""
        x_t, noise = _f32c(x_t), _f32c(noise)
        t = self._ddpm_t(t, x_t)
        out = torch.empty_like(x_t)
        B = x_t.shape[0]
        launch_ddpm_step(self._ddpm_dev(x_t.device)["coef"], t, B=B, per=x_t.numel() // B, x=x_t, eps_c=noise, x_recon=out, flags=0)
        return out

    @torch.no_grad()
    def q_posterior(self, x_start, x_t, t):
        """ddpm3d.py:218-225 -> (posterior_mean, posterior_variance, posterior_log_variance_clipped)"""
        x_start, x_t = _f32c(x_start), _f32c(x_t)
        t = self._ddpm_t(t, x_t)
        mean = torch.empty_like(x_t)
        B = x_t.shape[0]
        launch_ddpm_step(self._ddpm_dev(x_t.device)["coef"], t, B=B, per=x_t.numel() // B, x=x_t, eps_c=x_start, mean=mean,
                         flags=_l.MOCA_DDPM_X0)
        return mean, self._extract("posterior_variance", t, x_t), self._extract("posterior_log_variance_clipped", t, x_t)

    def _ddpm_step(self, x, c, t, clip_denoised, *, want_out, want_recon=False, want_mean=False, noise=None, repeat_noise=False,
                   temperature=1., mask=None, x0=None, noise_q=None, unconditional_guidance_scale=1., unconditional_conditioning=None,
                   score_corrector=None, corrector_kwargs=None, **kwargs):
        """UNet call(s) + ONE launch of the kernel: p_mean_variance (:565-588), the draw and update of p_sample (:601-610) and, with
        `mask`, the blend of the loop (:646-648).  -> (out, x_recon, mean), None where not asked for"""
        if score_corrector is not None:
            raise NotImplementedError("score_corrector is outside the DDPM sampler's scope")
        x = _f32c(x)
        t = self._ddpm_t(t, x)
        B = x.shape[0]
        scale = 1.0 if unconditional_guidance_scale is None else float(unconditional_guidance_scale)
        uc = unconditional_conditioning if scale != 1. else None
        # the guidance branches share the UNet prefix exactly where the one-graph step does (and only without further UNet kwargs);
        # otherwise one apply_model per branch (:567).  The kernel combines them
        e = guidance_eps(self, x, t, c, uc, scale, share_prefix=uc is not None and not kwargs and DdpmEngine.supported(self, x, c, uc),
                         share_any=True, batch=False, **kwargs)
        eps_c, eps_u = (_f32c(e), None) if torch.is_tensor(e) else (_f32c(e[0]), _f32c(e[1]))
        out = recon = mean = None
        if want_out:
            out = torch.empty_like(x)
            if noise is None:                                                                # noise_like, common.py:31-34
                noise = torch.randn((1,) + tuple(x.shape[1:]), device=x.device).repeat(B, *((1,) * (x.dim() - 1))) if repeat_noise \
                    else torch.randn(x.shape, device=x.device)
            noise = _f32c(noise.to(x.device))
            if noise.shape != x.shape:
                raise ValueError(f"noise {tuple(noise.shape)} does not match x {tuple(x.shape)}")
        recon = torch.empty_like(x) if want_recon else None
        mean = torch.empty_like(x) if want_mean else None
        flags = self._ddpm_flags(clip=clip_denoised)
        mask_inner = 0
        if mask is not None:
            mask, mflag, mask_inner = mask_operand(mask, x.shape, x.device)
            flags |= mflag
            x0 = _f32c(x0.to(x.device))
            noise_q = torch.randn_like(x0) if noise_q is None else _f32c(noise_q.to(x.device))         # q_sample's default draw, :413
        launch_ddpm_step(self._ddpm_dev(x.device)["coef"], t, B=B, per=x.numel() // B, x=x, out=out, eps_c=eps_c, eps_u=eps_u,
                         noise=noise if want_out else None, x_recon=recon, mean=mean, mask=mask, x0=x0 if mask is not None else None,
                         noise_q=noise_q if mask is not None else None, mask_inner=mask_inner, cfg_scale=scale,
                         temperature=temperature, flags=flags)
        return out, recon, mean

    @torch.no_grad()
    def p_mean_variance(self, x, c, t, clip_denoised: bool, return_x0=False, score_corrector=None, corrector_kwargs=None, **kwargs):
        """ddpm3d.py:565-588 -> (model_mean, posterior_variance, posterior_log_variance[, x_recon])"""
        _, recon, mean = self._ddpm_step(x, c, t, clip_denoised, want_out=False, want_recon=return_x0, want_mean=True,
                                         score_corrector=score_corrector, corrector_kwargs=corrector_kwargs, **kwargs)
        td = torch.as_tensor(t).to(mean.device, torch.int64)
        pv, plv = self._extract("posterior_variance", td, mean), self._extract("posterior_log_variance_clipped", td, mean)
        return (mean, pv, plv, recon) if return_x0 else (mean, pv, plv)

    @torch.no_grad()
    def p_sample(self, x, c, t, clip_denoised=False, repeat_noise=False, return_x0=False, temperature=1., noise_dropout=0.,
                 score_corrector=None, corrector_kwargs=None, noise=None, **kwargs):
        """ddpm3d.py:591-610.  `t` is per sample; a batch may mix t == 0 (no noise) with t > 0.  `noise=` fixes the draw."""
        if noise_dropout > 0.:
            raise NotImplementedError("noise_dropout is outside the DDPM sampler's scope")
        out, recon, _ = self._ddpm_step(x, c, t, clip_denoised, want_out=True, want_recon=return_x0, noise=noise,
                                        repeat_noise=repeat_noise, temperature=temperature, score_corrector=score_corrector,
                                        corrector_kwargs=corrector_kwargs, **kwargs)
        return (out, recon) if return_x0 else out

    # ---- the loop --------------------------------------------------------------------------------------------------------------
    def _ddpm_engine_for(self, img, cond, uc, scale, timesteps, mask, x0, seed):
        key = DdpmEngine.key(img.shape, cond, uc, timesteps, scale, mask, self.clip_denoised, self.parameterization, img.device)
        return self._ddpm_engines.get(key, lambda: DdpmEngine(self, img, cond, uc, scale, timesteps, mask=mask, x0=x0, seed=seed),
                                      lambda eng: eng.reset(img, cond, uc, seed, mask=mask, x0=x0))

    def release(self):
        """free the cached step graph of `p_sample_loop` (plan buffers + hipGraph)"""
        self._ddpm_engines.release()

    @torch.no_grad()
    def p_sample_loop(self, cond, shape, return_intermediates=False, x_T=None, verbose=True, callback=None, timesteps=None, mask=None,
                      x0=None, img_callback=None, start_T=None, log_every_t=None, noises=None, mask_noises=None,
                      unconditional_guidance_scale=1.0, unconditional_conditioning=None, use_graph=None, **kwargs):
        """ddpm3d.py:613-657: `timesteps` (capped by `start_T`) calls of p_sample from i = timesteps - 1 down to 0 with
        `clip_denoised=self.clip_denoised`; with `mask`, every step ends in `img = q_sample(x0, ts) * mask + (1 - mask) * img`.
        Extensions (defaults reproduce the reference): `noises[k]` / `mask_noises[k]` fix step k's two draws;
        `unconditional_guidance_scale` / `unconditional_conditioning`: classifier-free guidance (ddim.py:304), which the reference's
        loop does not have; `use_graph` None / True: one hipGraph per step (`fifo_graph.DdpmEngine`) where the call allows it
        ('crossattn' with `c_crossattn` / `fps` only, no further p_sample kwargs), False: the host-issued loop."""
        if not log_every_t:
            log_every_t = self.log_every_t
        device = self.betas.device
        b = shape[0]
        img = torch.randn(tuple(shape), device=device) if x_T is None else x_T
        intermediates = [img]
        if timesteps is None:
            timesteps = self.num_timesteps
        if start_T is not None:
            timesteps = min(timesteps, start_T)
        if mask is not None:
            assert x0 is not None
            assert x0.shape[2:3] == mask.shape[2:3]  # spatial size has to match
        if kwargs.get("noise_dropout", 0.) > 0.:
            raise NotImplementedError("noise_dropout is outside the DDPM sampler's scope")
        scale = 1.0 if unconditional_guidance_scale is None else float(unconditional_guidance_scale)
        uc = unconditional_conditioning if scale != 1. else None
        if use_graph is not False and timesteps > 0 and not kwargs and DdpmEngine.supported(self, img, cond, uc):
            key = conditioning_key(self)
            cd = as_cond_dict(cond, key)
            ud = None if uc is None else as_cond_dict(uc, key)
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())                  # the host generator seeds the device stream
            eng = self._ddpm_engine_for(img, cd, ud, scale, timesteps, mask, x0, seed)
            for k, i in enumerate(reversed(range(0, timesteps))):
                eng.step(noise=None if noises is None else noises[k], mask_noise=None if mask_noises is None else mask_noises[k])
                log = i % log_every_t == 0 or i == timesteps - 1
                if log or img_callback:
                    img = eng.latents().to(img.dtype)
                if log:
                    intermediates.append(img)
                if callback: callback(i)
                if img_callback: img_callback(img, i)
            return (img, intermediates) if return_intermediates else img      # (i == 0 is always logged: img is the last step's)
        for k, i in enumerate(reversed(range(0, timesteps))):
            ts = torch.full((b,), i, device=device, dtype=torch.long)
            img, _, _ = self._ddpm_step(img, cond, ts, self.clip_denoised, want_out=True, noise=None if noises is None else noises[k],
                                        mask=mask, x0=x0, noise_q=None if mask_noises is None else mask_noises[k],
                                        unconditional_guidance_scale=scale, unconditional_conditioning=uc,
                                        **{n: v for n, v in kwargs.items() if n != "noise_dropout"})
            if i % log_every_t == 0 or i == timesteps - 1:
                intermediates.append(img)
            if callback: callback(i)
            if img_callback: img_callback(img, i)
        if return_intermediates:
            return img, intermediates
        return img


for _n in TABLE_NAMES:
    setattr(DdpmMixin, _n, _table_property(_n))
