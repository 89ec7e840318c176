"""MI355X host-side mirror of `lvdm.models.samplers.ddim.DDIMSampler` for the hot path:
`make_schedule` (ddim.py:62-106), `sample`/`ddim_sampling` (:109-252), `p_sample_ddim`
(:274-359), `fifo_onestep` (:255-271), `unet` (:362-374), the MoCA `ddim_step`
(:377-649) and the start-from-a-video path: `stochastic_encode` (:652-671), `decode` (:674-692),
`ddim_inversion` (:972-1032) and `encode`, the deterministic DDIM inversion that upstream's sampler keeps beside them.  All per-element arithmetic runs in the fp32 HIP kernels of
csrc/sampler.hip; only O(steps) scalar schedule math stays on the host (numpy, as in
the reference).

Differences from the reference, all explicit:
  * noise is an optional explicit argument everywhere (the reference draws torch.randn
    inside: ddim.py:345,561) so results are reproducible against fixtures;
  * the Grounded-SAM-2 mask producer (ddim.py:713-969) is out of scope: masks come in as
    tensors (`davis_masks`), no debug PNG/matplotlib dumps are written (:432-554,611-641);
  * the two CFG branches are evaluated as ONE batched UNet call when their contexts have
    the same length (bit-equivalent: every UNet op is per-sample);
  * `sample` / `decode` implement `mask=` / `x0=`, which the reference declares (ddim.py:109-190) and never reads: the blend of the
    upstream latent-diffusion DDIM loop in front of every step (`moca_ddpm_step_f32` without eps: the blend alone).
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import lib as _l
from . import ops
from .conditioning import _f32c, check_schedule_index, cond_image_rows, guidance_eps
from .fifo_graph import (BaseEngine, DpmEngine, EngineCache, InvertEngine, ddim_coef, dpm_stepped_rows, dpmpp_tables, invert_coef,
                         mask_operand, state_block)


def make_ddim_timesteps(ddim_discr_method, num_ddim_timesteps, num_ddpm_timesteps, verbose=True):
    """utils_diffusion.py:56-78"""
    if ddim_discr_method == 'uniform':
        ddim_timesteps = np.linspace(0, num_ddpm_timesteps - 1, num_ddim_timesteps).round().copy().astype(np.int64)
        steps_out = ddim_timesteps
    elif ddim_discr_method == 'quad':
        ddim_timesteps = ((np.linspace(0, np.sqrt(num_ddpm_timesteps * .8), num_ddim_timesteps)) ** 2).astype(int)
        steps_out = ddim_timesteps + 1
    else:
        raise NotImplementedError(f'There is no ddim discretization method called "{ddim_discr_method}"')
    if verbose:
        print(f'Selected timesteps for ddim sampler: {steps_out}')
    return steps_out


def make_ddim_sampling_parameters(alphacums, ddim_timesteps, eta, verbose=True):
    """utils_diffusion.py:81-93"""
    alphas = alphacums[ddim_timesteps]
    alphas_prev = np.asarray([alphacums[0]] + alphacums[ddim_timesteps[:-1]].tolist())
    sigmas = eta * np.sqrt((1 - alphas_prev) / (1 - alphas) * (1 - alphas / alphas_prev))
    return sigmas, alphas, alphas_prev


def sqrt_f32(t):
    """fp32 square root of a host tensor, correctly rounded on every host (numpy's: the hardware instruction).  torch's own CPU sqrt /
    `** 0.5` is not correctly rounded and its last bit differs between CPU vendors (an Intel and an AMD EPYC host disagree on a fifth
    of the 1000 `alphas_cumprod`), so schedule coefficients taken with it -- and the latents they scale -- would depend on the host;
    the reference's `torch.sqrt(ddim_alphas)` / `alpha ** 0.5` mean this value."""
    t = torch.as_tensor(t, dtype=torch.float32).detach().cpu().contiguous()
    return torch.from_numpy(np.sqrt(t.numpy()))


def _st():
    return C.c_void_p(ops.current_stream())


def cfg_combine(e, scale):
    """e_u + s (e_c - e_u) (ddim.py:304) of `guidance_eps`'s answer, one launch; a single eps (no guidance) as it is"""
    if torch.is_tensor(e):
        return e
    e_c, e_u = _f32c(e[0]), _f32c(e[1])
    out = torch.empty_like(e_c)
    _l.check(_l.load().moca_cfg_combine_f32(_l.ptr(e_c), _l.ptr(e_u), _l.ptr(out), float(scale), e_c.numel(), _st()), "moca_cfg_combine_f32")
    return out


def noise_queue(z, alphas_per_frame, frame_index, noises):
    """The noising queue of `prepare_latents` (funcs.py:53-79) and `ddim_inversion` (ddim.py:1008-1022) as one launch: output frame j =
    alpha_j ** 0.5 * z[:, :, frame_index[j]] + (1 - alpha_j) ** 0.5 * eps_j over z [b,c,tz,h,w] (cuda, fp32).  The O(Q) coefficients are
    host scalars evaluated like the reference's 0-dim fp32 tensors (`sqrt_f32`: correctly rounded on every host).  `noises[j]`
    [b,c,1,h,w] fix the draws, else one torch.randn stands for the Q torch.randn_like calls of the reference."""
    b, c, tz, h, w = z.shape
    alphas = torch.as_tensor(alphas_per_frame, dtype=torch.float32)
    Q = alphas.shape[0]
    coef_z, coef_n = sqrt_f32(alphas), sqrt_f32(1 - alphas)
    fidx = torch.as_tensor(frame_index, dtype=torch.int32)
    if noises is None:
        noise = torch.randn(b, c, Q, h, w, device=z.device)
    else:
        noise = torch.cat([n.to(z.device, torch.float32).reshape(b, c, 1, h, w) for n in noises[:Q]], dim=2).contiguous()
    out = torch.empty(b, c, Q, h, w, dtype=torch.float32, device=z.device)
    cz, cn, fi = coef_z.to(z.device), coef_n.to(z.device), fidx.to(z.device)      # (named: a temporary's block would be reused by the next)
    _l.check(_l.load().moca_fifo_prepare_queue_f32(_l.ptr(z), _l.ptr(noise), _l.ptr(out), _l.ptr(cz), _l.ptr(cn), _l.ptr(fi), b * c, tz, Q,
                                                   h * w, _st()), "moca_fifo_prepare_queue_f32")
    return out


def check_inpaint(shape, mask, x0):
    """the argument contract of masked sampling over latents of `shape`: `mask` and `x0` come together, `x0` has the latents' shape,
    `mask` broadcasts against them (ValueError otherwise) -> whether the call is masked"""
    if (mask is None) != (x0 is None):
        raise ValueError("mask= and x0= go together: the mask says where x0 is kept (mask == 1) and where the sampler regenerates")
    if mask is None:
        return False
    shape = tuple(int(v) for v in shape)
    if tuple(x0.shape) != shape:
        raise ValueError(f"x0 {tuple(x0.shape)} does not have the latents' shape {shape}")
    ms = tuple(mask.shape)
    if len(ms) > len(shape) or any(m not in (1, v) for m, v in zip(ms[::-1], shape[::-1])):
        raise ValueError(f"mask {ms} does not broadcast against the latents {shape}")
    return True


class HostBlend:
    """The inpainting blend of the host-issued loops and of paste-back: `moca_ddpm_step_f32` without eps, the launch the masked step
    engines replay -- one kernel serves both, no torch arithmetic on latents.  `blend(x, timestep, noise_q)` rewrites x IN PLACE:
    x = q_sample(x0, timestep) mask + (1 - mask) x over the model's own DDPM table, `noise_q` None: drawn from the host generator.
    `blend.paste(x)` is the same launch on a private clean row (sac 1, s1mac 0, scale 1): orig = 1 x0 + 0 noise is x0 exactly, so
    where mask == 1 the result equals x0 bit for bit."""

    def __init__(self, model, x, mask, x0):
        dev = x.device
        self.model = model
        self.mask, self.mflag, self.inner = mask_operand(mask, x.shape, dev)
        self.x0 = _f32c(x0.to(dev))

    def _launch(self, x, coef, t, noise_q, flags):
        from .ddpm import launch_ddpm_step
        if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()):
            raise ValueError("the blend runs in place on contiguous fp32 cuda latents")
        B = x.shape[0]
        launch_ddpm_step(coef, t, B=B, per=x.numel() // B, x=x, out=x, mask=self.mask, x0=self.x0, noise_q=noise_q, mask_inner=self.inner,
                         flags=flags | self.mflag, t_stride=0)
        return x

    def __call__(self, x, timestep, noise_q=None):
        noise_q = torch.randn_like(x) if noise_q is None else _f32c(noise_q.to(x.device))        # q_sample's default draw, ddpm3d.py:413
        if noise_q.shape != x.shape:
            raise ValueError(f"mask noise {tuple(noise_q.shape)} does not match the latents {tuple(x.shape)}")
        t = torch.full((1,), int(timestep), dtype=torch.int64, device=x.device)
        return self._launch(x, self.model._ddpm_dev(x.device)["coef"], t, noise_q, self.model._ddpm_flags(x0_param=False))

    def paste(self, x):
        clean = torch.tensor([[0., 0., 0., 0., 0., 1., 0., 1.]], device=x.device)
        return self._launch(x, clean, torch.zeros(1, dtype=torch.int64, device=x.device), torch.zeros_like(x), 0)


class DDIMSampler(object):
    def __init__(self, model, schedule="linear", use_self_attention=False, **kwargs):
        self.model = model
        self.ddpm_num_timesteps = model.num_timesteps
        self.schedule = schedule
        self.counter = 0
        self.use_self_attention = use_self_attention
        self.reference_index_quirk = True    # see ddim_step
        self.cfg_mode = "batched"            # "batched": cond+uncond as one B=2 launch; "concurrent": two B=1
                                             # hipGraphs on two streams (UNetModel.forward_concurrent)
        self.beta = 0.9                      # momentum decay (ddim.py:397)
        self._engines = EngineCache()        # the step graph of `sample` / `decode`
        self.use_graph = True                # `sample`: one hipGraph per DDIM step (fifo_graph.BaseEngine) where the call allows it
        self.share_prefix = True             # the two CFG branches share everything before the first cross-attention (same x, same
                                             # t): computed once (UNetModel.forward_segments(shared_x=True)); False: plain B = 2 batch

    # ---- schedule (host) ---------------------------------------------------------------
    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0., verbose=True):
        self.ddim_timesteps = make_ddim_timesteps(ddim_discretize, ddim_num_steps, self.ddpm_num_timesteps, verbose=verbose)
        alphas_cumprod = self.model.alphas_cumprod
        assert alphas_cumprod.shape[0] == self.ddpm_num_timesteps, 'alphas have to be defined for each timestep'
        ac = alphas_cumprod.detach().cpu()
        self.use_scale = self.model.use_scale
        if self.use_scale:
            scale_arr = self.model.scale_arr.detach().cpu()
            self.ddim_scale_arr = scale_arr[self.ddim_timesteps]                                           # :82-83
            self.ddim_scale_arr_prev = np.asarray([scale_arr[0]] + scale_arr[self.ddim_timesteps[:-1]].tolist())  # :84-85
        sig, al, alp = make_ddim_sampling_parameters(alphacums=ac, ddim_timesteps=self.ddim_timesteps, eta=ddim_eta, verbose=verbose)
        self.ddim_sigmas, self.ddim_alphas, self.ddim_alphas_prev = sig, al, alp
        self.ddim_sqrt_one_minus_alphas = np.sqrt(1. - al)
        # q(x_t | x_0) tables over the DDPM steps (:89-90), read by stochastic_encode(use_original_steps=True): numpy's fp32 sqrt, like the reference's
        self.sqrt_alphas_cumprod = torch.as_tensor(np.sqrt(ac.numpy()), dtype=torch.float32)
        self.sqrt_one_minus_alphas_cumprod = torch.as_tensor(np.sqrt(1. - ac.numpy()), dtype=torch.float32)

    # ---- UNet with classifier-free guidance ----------------------------------------------
    def _cfg_eps(self, x, t, c, uc, scale, **kwargs):
        """e_u + s (e_c - e_u)  (ddim.py:290-304,362-374)"""
        e = guidance_eps(self.model, x, t, c, uc, scale, share_prefix=self.share_prefix, cfg_mode=self.cfg_mode, **kwargs)
        return cfg_combine(e, scale)

    @torch.no_grad()
    def unet(self, x, c, t, unconditional_guidance_scale=1., unconditional_conditioning=None, **kwargs):
        """ddim.py:362-374"""
        return self._cfg_eps(x, t, c, unconditional_conditioning, unconditional_guidance_scale, **kwargs)

    # ---- base DDIM step --------------------------------------------------------------------
    @torch.no_grad()
    def p_sample_ddim(self, x, c, t, index, repeat_noise=False, use_original_steps=False, quantize_denoised=False,
                      temperature=1., noise_dropout=0., score_corrector=None, corrector_kwargs=None,
                      unconditional_guidance_scale=1., unconditional_conditioning=None, uc_type=None,
                      conditional_guidance_scale_temporal=None, noise=None, **kwargs):
        """ddim.py:274-359 (uc_type None, no score corrector / temporal guidance / quantisation)"""
        if use_original_steps or quantize_denoised or score_corrector is not None or uc_type is not None \
                or conditional_guidance_scale_temporal is not None or noise_dropout > 0.:
            raise NotImplementedError("option outside the MoCA driver's call (funcs.py:223-236)")
        e_t = self._cfg_eps(x, t, c, unconditional_conditioning, unconditional_guidance_scale, **kwargs)
        return self.ddim_update(x, e_t, index, noise=noise, temperature=temperature)

    def ddim_update(self, x, e_t, index, noise=None, temperature=1.):
        """the arithmetic tail of p_sample_ddim (ddim.py:328-357) on the HIP kernel"""
        x, e_t = _f32c(x), _f32c(e_t)
        if noise is None:
            noise = torch.randn(x.shape, device=x.device)          # noise_like, common.py:31-34
        noise = _f32c(noise)
        if temperature != 1.:
            noise = noise * temperature
        x_prev, pred_x0 = torch.empty_like(x), torch.empty_like(x)
        f32 = np.float32
        use_scale = bool(self.use_scale)
        _l.check(_l.load().moca_ddim_update_f32(
            _l.ptr(x), _l.ptr(e_t), _l.ptr(noise), _l.ptr(x_prev), _l.ptr(pred_x0),
            f32(self.ddim_alphas[index]), f32(self.ddim_alphas_prev[index]), f32(self.ddim_sigmas[index]),
            f32(self.ddim_sqrt_one_minus_alphas[index]), 1 if use_scale else 0,
            f32(self.ddim_scale_arr[index]) if use_scale else f32(1), f32(self.ddim_scale_arr_prev[index]) if use_scale else f32(1),
            x.numel(), _st()), "moca_ddim_update_f32")
        return x_prev, pred_x0

    def _engine_for(self, img, cond, uc, scale, seed, n_rows, features_adapter=None, mask=None, x0=None):
        """the cached step graph (fifo_graph.BaseEngine) for this call, reset to a new trajectory; built when `BaseEngine.key` changes.
        `n_rows`: the rows of the schedule tables the captured kernels index (all of them for `sample`, the first t_start for `decode`);
        `mask` / `x0`: a masked engine (another mask that is read the same way reuses it)"""
        return self._engines.get(BaseEngine.key(self, img, cond, uc, scale, features_adapter, n_rows, mask),
                                 lambda: BaseEngine(self.model, self, img, cond, uc, scale, seed=seed, features_adapter=features_adapter,
                                                    n_rows=n_rows, mask=mask, x0=x0),
                                 lambda eng: eng.reset(img, cond, uc, seed, features_adapter=features_adapter, mask=mask, x0=x0))

    _base_engine = property(lambda self: self._engines.entry, doc="None, or the (key, engine) of the cached step graph")

    def release(self):
        """free the cached step graph of `sample` (plan buffers + hipGraph)"""
        self._engines.release()

    def _run_steps(self, x, cond, uc, scale, n_steps, noises, use_graph, features_adapter=None, mask=None, x0=None, mask_noises=None):
        """the loop of `sample` and `decode`: n_steps calls of p_sample_ddim over `ddim_timesteps[:n_steps]` flipped -- step i at schedule
        index n_steps - 1 - i, `noises[i]` fixing its draw -- as one hipGraph per step (fifo_graph.BaseEngine: latents, schedule and
        noise stay on the device) where `use_graph` and `BaseEngine.supported` allow it, else host-issued.  With `mask` / `x0`
        (`check_inpaint` has seen them) every step starts with upstream's blend, x = q_sample(x0, t) mask + (1 - mask) x, `mask_noises[i]`
        fixing its draw: inside the masked engine's graph, or `HostBlend` in front of the host-issued step."""
        noise = lambda i: None if noises is None else noises[i]
        mask_noise = lambda i: None if mask_noises is None else mask_noises[i]
        if n_steps > 0 and use_graph and self.share_prefix and BaseEngine.supported(self.model, x, cond, uc, scale,
                                                                                    features_adapter=features_adapter):
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())                  # the host generator seeds the device stream
            eng = self._engine_for(x, cond, uc, scale, seed, n_steps, features_adapter=features_adapter, mask=mask, x0=x0)
            for i in range(n_steps):
                eng.step(noise=noise(i), **({} if mask is None else {"mask_noise": mask_noise(i)}))
            return eng.latents().to(x.dtype)
        unet_kwargs = {} if features_adapter is None else {"features_adapter": list(features_adapter)}
        blend = None
        if mask is not None and n_steps > 0:
            x = _f32c(x).clone()                                                 # (the blend runs in place: the caller keeps x_T)
            blend = HostBlend(self.model, x, mask, x0)
        for i, step in enumerate(np.flip(self.ddim_timesteps[:n_steps])):
            if blend is not None:
                x = blend(_f32c(x), int(step), mask_noise(i))
            ts = torch.full((x.shape[0],), int(step), device=x.device, dtype=torch.long)
            x, _ = self.p_sample_ddim(x, cond, ts, index=n_steps - i - 1, use_original_steps=False, unconditional_guidance_scale=scale,
                                      unconditional_conditioning=uc, noise=noise(i), **unet_kwargs)
        return x

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, eta=0., x_T=None, verbose=False,
               unconditional_guidance_scale=1., unconditional_conditioning=None, latents_dir=None, noises=None,
               features_adapter=None, mask=None, x0=None, mask_noises=None, **kwargs):
        """ddim.py:109-181 -> ddim_sampling (:183-252): the base 'N DDIM steps, single prompt' loop.  `features_adapter` (a list of
        maps, entry k [batch*T, C_k, h_k, w_k]) is what the reference's `sample(**kwargs)` hands down to `apply_model` and the UNet
        (openaimodel3d.py:562-567): constant over the trajectory, the same for both guidance branches.

        `mask` / `x0`: masked inpainting as upstream's latent-diffusion DDIM loop has it (the reference declares both and never reads
        the mask): before the model call of every step, at the step's timestep t,
        `img = model.q_sample(x0, t) * mask + (1 - mask) * img` -- mask == 1 keeps x0, fresh q-noise every step (`mask_noises[i]` fixes
        step i's), nothing blended behind the last step, so the kept region of the result is one DDIM step away from x0 (pasting
        back is the driver's job, `fifo.inpaint_ddim_sampling`).  `x0` has the latents' shape, `mask` broadcasts against them."""
        self.make_schedule(ddim_num_steps=S, ddim_eta=eta, verbose=verbose)
        size = (batch_size,) + tuple(shape)
        check_inpaint(size, mask, x0)
        device = self.model.betas.device
        img = torch.randn(size, device=device) if x_T is None else x_T
        if latents_dir is not None:
            torch.save(img, f"{latents_dir}/0.pt")                    # :233-234
        total_steps = self.ddim_timesteps.shape[0]
        img = self._run_steps(img, conditioning, unconditional_conditioning, unconditional_guidance_scale, total_steps, noises, self.use_graph,
                              features_adapter=features_adapter, mask=mask, x0=x0, mask_noises=mask_noises)
        if latents_dir is not None:
            torch.save(img, f"{latents_dir}/{total_steps}.pt")        # :249-250
        return img, {}

    @torch.no_grad()
    def sample_freeinit(self, steps, batch_size, shape, LPF, conditioning=None, eta=0., x_T=None, z_rands=None, noises=None,
                        unconditional_guidance_scale=1., unconditional_conditioning=None, features_adapter=None, return_all=False,
                        verbose=False):
        """FreeInit (Wu et al., 2023) over `sample`: len(steps) trajectories of steps[k] DDIM steps (`freeinit.freeinit_steps`; the last
        is the longest); trajectory 0 starts from the initial noise (`x_T`, else drawn), every later one from the previous samples
        re-noised to the last timestep with that SAME initial noise and mixed with fresh noise under the low-pass filter `LPF`
        (`freeinit.freeinit_reinit`).  `z_rands[k-1]` fixes the fresh noise of trajectory k, `noises[k][i]` the draw of its step i.

        Where `sample` runs on the step graph, the whole run stays on ONE cached engine, captured for steps[-1] rows: `reset` at the
        start, `BaseEngine.set_schedule` where the step count changes (no new capture), `BaseEngine.reinit` between trajectories (latents,
        initial noise, filter and fresh noise stay on the device), one read-back at the end -- one per trajectory with `return_all`.
        Elsewhere the same loop is composed on the host from `freeinit_reinit` and host-issued steps.
        Takes no `mask=` / `x0=`: masked inpainting across re-initialised trajectories is out of scope (`sample` and `decode` have it).
        Returns (samples of the last trajectory, the list of every trajectory's samples or None)."""
        from .freeinit import freeinit_reinit
        steps = [int(s) for s in steps]
        if not steps or max(steps) != steps[-1] or min(steps) < 1:
            raise ValueError(f"steps = {steps}: at least one trajectory, every one of 1 .. steps[-1] steps")
        if z_rands is not None and len(z_rands) != len(steps) - 1:
            raise ValueError(f"z_rands holds {len(z_rands)} tensors for {len(steps) - 1} re-initialisations")
        if noises is not None and len(noises) != len(steps):
            raise ValueError(f"noises holds {len(noises)} lists for {len(steps)} trajectories")
        cond, uc, scale = conditioning, unconditional_conditioning, unconditional_guidance_scale
        self.make_schedule(ddim_num_steps=steps[-1], ddim_eta=eta, verbose=verbose)
        device = self.model.betas.device
        initial_noise = torch.randn((batch_size,) + tuple(shape), device=device) if x_T is None else x_T
        z_rand = lambda k: None if z_rands is None else z_rands[k - 1]
        noise = lambda k, i: None if noises is None else noises[k][i]
        new_seed = lambda: int(torch.randint(0, 2 ** 62, (1,)).item())          # the host generator seeds the device streams
        every = []
        if self.use_graph and self.share_prefix and BaseEngine.supported(self.model, initial_noise, cond, uc, scale,
                                                                          features_adapter=features_adapter):
            eng = self._engine_for(initial_noise, cond, uc, scale, new_seed(), steps[-1], features_adapter=features_adapter)
            for k, S in enumerate(steps):
                if S != eng.S - eng.it0:                                          # (the engine's schedule is the sampler's throughout)
                    self.make_schedule(ddim_num_steps=S, ddim_eta=eta, verbose=verbose)
                    eng.set_schedule(self)
                if k > 0:
                    eng.reinit(initial_noise, LPF, z_rand=z_rand(k), seed=new_seed())
                for i in range(S):
                    eng.step(noise=noise(k, i))
                if return_all:
                    every.append(eng.latents().to(initial_noise.dtype))
            x = every[-1] if return_all else eng.latents().to(initial_noise.dtype)
            return x, (every if return_all else None)
        unet_kwargs = dict(features_adapter=features_adapter)
        x = initial_noise
        for k, S in enumerate(steps):
            if k > 0:
                zr = z_rand(k)
                x = freeinit_reinit(self.model, x, initial_noise, torch.randn_like(initial_noise, dtype=torch.float32) if zr is None else zr, LPF)
            self.make_schedule(ddim_num_steps=S, ddim_eta=eta, verbose=verbose)
            x = self._run_steps(x, cond, uc, scale, S, None if noises is None else noises[k], False, **unet_kwargs)
            every.append(x)
        return x, (every if return_all else None)

    # ---- start from an existing latent: noise it, denoise it ---------------------------------------------------------------
    def encode_tables(self, use_original_steps=False):
        """the two coefficient tables of `stochastic_encode` (ddim.py:655-660) as fp32 host tensors, evaluated as the reference evaluates
        them: `torch.sqrt(ddim_alphas)` (taken with `sqrt_f32`: the same on every host) and `ddim_sqrt_one_minus_alphas` over the DDIM
        steps, or the sampler's own 1000-entry `sqrt_alphas_cumprod` / `sqrt_one_minus_alphas_cumprod` (:89-90).  `scale_arr` plays no
        part, `use_scale` or not."""
        if use_original_steps:
            return self.sqrt_alphas_cumprod, self.sqrt_one_minus_alphas_cumprod
        return (sqrt_f32(np.asarray(self.ddim_alphas)),
                torch.as_tensor(np.asarray(self.ddim_sqrt_one_minus_alphas), dtype=torch.float32))

    @torch.no_grad()
    def stochastic_encode(self, x0, t, use_original_steps=False, noise=None):
        """ddim.py:652-671: x_t = a[t_b] x0 + b[t_b] noise per sample b.  `t` [B] holds schedule INDICES (into the DDIM tables, or into
        the 1000 DDPM steps with `use_original_steps`), on either device: a host tensor is range-checked here (IndexError, as `gather`),
        a device tensor is gathered by the kernel without a host read (an index out of range gives that sample NaN)."""
        x0 = _f32c(x0)
        if not x0.is_cuda:
            raise ValueError("stochastic_encode runs on the GPU: x0 must be a cuda tensor")
        ca, cb = self.encode_tables(use_original_steps)
        B = x0.shape[0]
        t = check_schedule_index(t, B, ca.shape[0])
        noise = torch.randn_like(x0) if noise is None else _f32c(noise.to(x0.device))                    # :662-663
        if noise.shape != x0.shape:
            raise ValueError(f"noise {tuple(noise.shape)} does not match x0 {tuple(x0.shape)}")
        ca_d, cb_d, t_d = ca.to(x0.device), cb.to(x0.device), t.to(x0.device, torch.int64).contiguous()
        out = torch.empty_like(x0)
        _l.check(_l.load().moca_q_sample_f32(_l.ptr(x0), _l.ptr(noise), _l.ptr(out), _l.ptr(ca_d), _l.ptr(cb_d), _l.ptr(t_d), B,
                                             int(ca.shape[0]), x0.numel() // B, _st()), "moca_q_sample_f32")
        return out

    @torch.no_grad()
    def decode(self, x_latent, cond, t_start, unconditional_guidance_scale=1.0, unconditional_conditioning=None,
               use_original_steps=False, noises=None, use_graph=None, mask=None, x0=None, mask_noises=None):
        """ddim.py:674-692: `t_start` calls of p_sample_ddim (temperature 1, fresh noise per step) over `ddim_timesteps[:t_start]`
        flipped -- step i at schedule index t_start - 1 - i -- returning the latents only.  `noises[i]` fixes step i's draw; `use_graph`
        (default: `self.use_graph`) as in `sample`: where `BaseEngine.supported` holds, one hipGraph per step on an engine over the first
        t_start rows of the schedule tables, else (no guidance pair among the rest) the host-issued p_sample_ddim loop.  `mask` / `x0` /
        `mask_noises`: `sample`'s blend in front of every step."""
        check_inpaint(x_latent.shape, mask, x0)
        if use_original_steps:
            raise NotImplementedError(
                "decode(use_original_steps=True) cannot run in the reference: p_sample_ddim reads self.model.ddim_sigmas_for_original_num_steps "
                "(ddim.py:325), which exists only on the sampler, and self.model.scale_arr_prev (ddim.py:352), which is never registered")
        n_steps = self.ddim_timesteps[:t_start].shape[0]              # :677-678 (numpy slicing: a t_start past the schedule is the whole of it)
        return self._run_steps(x_latent, cond, unconditional_conditioning, unconditional_guidance_scale, n_steps, noises,
                               self.use_graph if use_graph is None else use_graph, mask=mask, x0=x0, mask_noises=mask_noises)

    def _invert_engine_for(self, x0, cond, uc, scale):
        """the cached step graph of `encode` (fifo_graph.InvertEngine) reset to the clip `x0`; built when `InvertEngine.key` changes.  It
        shares the one-entry cache of `sample` / `decode`."""
        uc = uc if scale != 1.0 else None
        return self._engines.get(InvertEngine.key(self, x0, cond, uc, scale), lambda: InvertEngine(self.model, self, x0, cond, uc, scale),
                                 lambda eng: eng.reset(x0, cond, uc))

    def invert_update(self, x, e_t, i, zeros=None):
        """inversion step `i` of `encode` on the host-issued path: `moca_ddim_update_f32` with the scalars of `invert_coef` -- the
        alphas and scales swapped, sigma 0 -- and a noise operand of zeros (`zeros`, else made here).  Draws nothing.
        Returns (x_next, pred_x0)."""
        x, e_t = _f32c(x), _f32c(e_t)
        zeros = torch.zeros_like(x) if zeros is None else zeros
        x_next, pred_x0 = torch.empty_like(x), torch.empty_like(x)
        f32 = np.float32
        _, _, sigma, s1m_cur, _, s_cur, s_next = invert_coef(self, i)
        _l.check(_l.load().moca_ddim_update_f32(
            _l.ptr(x), _l.ptr(e_t), _l.ptr(zeros), _l.ptr(x_next), _l.ptr(pred_x0),
            f32(self.ddim_alphas_prev[i]), f32(self.ddim_alphas[i]), sigma, s1m_cur, 1 if self.use_scale else 0, s_cur, s_next,
            x.numel(), _st()), "moca_ddim_update_f32")
        return x_next, pred_x0

    def _encode_host(self, x0, c, t_enc, uc, scale, inter=None, callback=None):
        """the host-issued loop of `encode`: step i evaluates the model at ddim_timesteps[i] (`_cfg_eps`) and updates with the
        coefficients of level index i (`invert_update`), one zero tensor serving every step as the noise operand"""
        x = _f32c(x0)
        zeros = torch.zeros_like(x)
        for i in range(t_enc):
            ts = torch.full((x.shape[0],), int(self.ddim_timesteps[i]), device=x.device, dtype=torch.long)
            e_t = self._cfg_eps(x, ts, c, uc, scale)
            x, _ = self.invert_update(x, e_t, i, zeros)
            if inter is not None:
                inter.append(x)
            if callback is not None:
                callback(i)
        return x

    @torch.no_grad()
    def encode(self, x0, c, t_enc, use_original_steps=False, return_intermediates=None, unconditional_guidance_scale=1.0,
               unconditional_conditioning=None, callback=None, use_graph=None):
        """Deterministic DDIM inversion, the `encode` of upstream's sampler (same parameters, in its order; `use_graph` is ours, as in
        `decode`): t_enc steps i = 0 .. t_enc - 1, step i taking the latents from schedule level ddim_alphas_prev[i] to ddim_alphas[i]
        with the model evaluated at t = ddim_timesteps[i]:

            e       = e_u + g (e_c - e_u)                      (g = 1 or no unconditional conditioning: e = e_c, one UNet call)
            pred_x0 = (x - sqrt(1 - a_cur) e) / sqrt(a_cur) [/ s_cur]
            x_next  = sqrt(a_next) [s_next] pred_x0 + sqrt(1 - a_next) e

        -- the tail of p_sample_ddim (ddim.py:328-357) with its tables swapped and sigma 0 (`invert_coef`); without `use_scale` upstream's
        own formula.  After step i the state is at level ddim_alphas[i], where `decode(x, c, t_start=i + 1)` starts:
        `decode(encode(x0, c, n)[0], c, n)` at eta 0 is a round trip.  Draws nothing: the host generator is left as it was.

        Returns (x_T, out): out["x_encoded_steps"] = t_enc and, with `return_intermediates`, out["intermediates"] = the t_enc states
        after each step and out["intermediate_steps"] = their timesteps.  `callback(i)` runs after step i.  Where `use_graph` (default:
        `self.use_graph`) and `InvertEngine.supported` allow it every step is one hipGraph and the latents stay on the device; else
        host-issued: `_cfg_eps` and `moca_ddim_update_f32`."""
        if use_original_steps:
            raise NotImplementedError("encode(use_original_steps=True): inversion over the 1000 DDPM steps is not built; like "
                                      "decode(use_original_steps=True) it has no tables to run on here")
        S = len(self.ddim_timesteps)
        if isinstance(t_enc, bool) or int(t_enc) != t_enc or not 1 <= int(t_enc) <= S:
            raise ValueError(f"t_enc = {t_enc}: inversion takes 1 .. {S} steps of the {S}-step schedule")
        t_enc = int(t_enc)
        if not (torch.is_tensor(x0) and x0.is_cuda):
            raise ValueError("encode runs on the GPU: x0 must be a cuda tensor")
        uc, scale = unconditional_conditioning, unconditional_guidance_scale
        guided = uc is not None and scale != 1.0
        use_graph = self.use_graph if use_graph is None else use_graph
        inter = [] if return_intermediates else None
        if use_graph and (self.share_prefix or not guided) and InvertEngine.supported(self.model, x0, c, uc, scale):
            eng = self._invert_engine_for(x0, c, uc, scale)
            for i in range(t_enc):
                eng.step()
                if inter is not None:
                    inter.append(eng.latents().to(x0.dtype))
                if callback is not None:
                    callback(i)
            x = inter[-1] if inter is not None else eng.latents().to(x0.dtype)
        else:
            x = self._encode_host(x0, c, t_enc, uc, scale, inter, callback).to(x0.dtype)
        out = {"x_encoded_steps": t_enc}
        if inter is not None:
            out.update(intermediates=inter, intermediate_steps=[int(t) for t in self.ddim_timesteps[:t_enc]])
        return x, out

    @staticmethod
    def inversion_frame_index(num_inference_steps, n_frames):
        """ddim.py:1014: the input frame behind output frame i, idx(i) = max(0, i - (num_inference_steps - n_frames))"""
        return [max(0, i - (num_inference_steps - n_frames)) for i in range(num_inference_steps)]

    @torch.no_grad()
    def ddim_inversion(self, frames, num_inference_steps, eta=1.0, latents_dir=None, noises=None, anchor_noise=None,
                       deterministic=False, cond=None, unconditional_guidance_scale=1.0, unconditional_conditioning=None):
        """ddim.py:972-1032.  Noising by default, inversion with `deterministic=True`.  By default, despite the name, a NOISING queue: output frame i = ddim_alphas[i] ** 0.5 * z[:, :, idx(i)] +
        (1 - ddim_alphas[i]) ** 0.5 * randn with z = encode_first_stage_2DAE(frames) (RGBA cut to RGB, a 3-channel z padded with a zero
        fourth channel) and idx(i) = max(0, i - (num_inference_steps - T)) -- `prepare_latents` (funcs.py:53-79) without lookahead over
        this sampler's tables, one `moca_fifo_prepare_queue_f32` launch.  `eta` is unused, as upstream; needs a prior `make_schedule`.
        `noises[i]` [B,C,1,h,w] fix the per-frame draws, `anchor_noise` [B,4,T,h,w] the VAE posterior draw.

        `deterministic=True`: the queue of the same shape taken from the clip's own DDIM inversion instead of from noise -- output frame
        i = X_i[:, :, idx(i)] with X_i the state after inversion step i of the whole clip z, i.e. z at level ddim_alphas[i], from
        `encode(z, cond, num_inference_steps, return_intermediates=True)` under `cond` (required) and the optional guidance pair.  Nothing
        is drawn but the VAE posterior sample, so `noises=` is refused.  The result goes into `fifo_ddim_sampling(latents=...)` like the
        noised queue; lookahead copies stay the caller's business."""
        if frames.dim() != 5:
            raise ValueError(f"Expected frames to have 5 dimensions [B, C, T, H, W], got {frames.dim()}")
        if deterministic and cond is None:
            raise ValueError("ddim_inversion(deterministic=True) evaluates the model: it needs cond=")
        if deterministic and noises is not None:
            raise ValueError("ddim_inversion(deterministic=True) draws no per-frame noise: noises= has nothing to fix")
        if frames.shape[1] == 4:                                      # RGBA -> RGB (:990-991)
            frames = frames[:, :3]
        kw = {} if anchor_noise is None else {"noise": anchor_noise}
        latents = self.model.encode_first_stage_2DAE(frames, **kw)
        if latents.dim() != 5:
            raise ValueError(f"Expected latents to have 5 dimensions [B, C, T, H, W], got {latents.dim()}")
        if latents.shape[1] == 3:                                     # :1001-1003
            latents = torch.cat([latents, torch.zeros_like(latents[:, :1])], dim=1)
        N = int(num_inference_steps)
        z = latents.to("cuda", torch.float32).contiguous()
        alphas = np.asarray(self.ddim_alphas)[:N]
        if alphas.shape[0] != N:
            raise IndexError(f"num_inference_steps = {N} runs past the {alphas.shape[0]}-step schedule (ddim.py:1010)")
        fidx = self.inversion_frame_index(N, frames.shape[2])
        if max(fidx) >= z.shape[2]:
            raise IndexError(f"frame index {max(fidx)} is out of range for {z.shape[2]} latent frames (ddim.py:1017)")
        if deterministic:
            _, enc = self.encode(z, cond, N, return_intermediates=True, unconditional_guidance_scale=unconditional_guidance_scale,
                                 unconditional_conditioning=unconditional_conditioning)
            out = torch.stack([x[:, :, j] for x, j in zip(enc["intermediates"], fidx)], dim=2)
        else:
            out = noise_queue(z, alphas, fidx, noises)
        if latents_dir is not None:
            for i in range(N):
                torch.save(out[:, :, [i]].clone(), f"{latents_dir}/step_{i}.pt")          # :1024-1025
        return out

    @torch.no_grad()
    def unet_windows(self, windows, c, ts_list, unconditional_guidance_scale=1., unconditional_conditioning=None, **kwargs):
        """CFG noise prediction for several independent FIFO windows in ONE batched UNet call.

        The 2n windows of one outer FIFO iteration read only pre-iteration frames (funcs.py:305-352: rank r
        writes [8r+8,8r+16) and rank r-1 reads [8r-8,8r+8)), so their UNet evaluations are independent; the
        reference's own multi-GPU variant relies on the same fact (funcs_mp.py:207-221).  Windows become the
        batch dimension with per-(window, frame) timesteps; with classifier-free guidance of equal context
        length the unconditional branch doubles the batch (2 x 2n = 16 videos per launch).  Returns the list of
        per-window eps tensors, equal to `self.unet(w, c, ts, ...)` per window."""
        W = len(windows)
        x = torch.cat(windows, 0)
        t = torch.cat([torch.as_tensor(np.asarray(ts).copy(), device=x.device).to(torch.long).reshape(-1) for ts in ts_list], 0)
        uc, scale = unconditional_conditioning, unconditional_guidance_scale
        fps_c = c.get("fps", 16)
        wide = lambda d, fps: {"c_crossattn": [k.expand(W, -1, -1) for k in d["c_crossattn"]], "fps": fps}    # one context per window
        e = guidance_eps(self.model, x, t, wide(c, fps_c), None if uc is None else wide(uc, uc.get("fps", fps_c)), scale,
                         share_prefix=self.share_prefix, rows=W, share_any=True, **kwargs)
        return list(cfg_combine(e, scale).split(1, 0))

    # ---- MoCA FIFO step -----------------------------------------------------------------------
    @torch.no_grad()
    def fifo_onestep(self, cond, shape, latents=None, timesteps=None, indices=None, unconditional_guidance_scale=1.,
                     unconditional_conditioning=None, cond_image=None, target=None, use_self_attention=False,
                     davis_masks=None, noise=None, sam_masks=None, sam_masks_fn=None, **kwargs):
        """ddim.py:255-271"""
        device = self.model.betas.device
        ts = torch.as_tensor(np.asarray(timesteps).copy(), device=device).to(dtype=torch.long)
        noise_pred = self.unet(latents, cond, ts, unconditional_guidance_scale=unconditional_guidance_scale,
                               unconditional_conditioning=unconditional_conditioning, **kwargs)
        return self.ddim_step(latents, noise_pred, indices, cond_image, target, ts, use_self_attention=use_self_attention,
                              davis_masks=davis_masks, noise=noise, sam_masks=sam_masks, sam_masks_fn=sam_masks_fn)

    @staticmethod
    def calculate_iou(masks1, masks2):
        """ddim.py:905-943: mean IoU over zip(masks1, masks2) of the masks binarised at 0.5 (both empty -> 1.0)"""
        m1, m2 = torch.as_tensor(masks1) > 0.5, torch.as_tensor(masks2) > 0.5
        ious = []
        for a, b in zip(m1, m2):
            b = b.to(a.device)
            inter, union = torch.logical_and(a, b).sum().float(), torch.logical_or(a, b).sum().float()
            ious.append(torch.tensor(1.0) if union == 0 else (inter / union).cpu())
        return torch.stack(ious).mean().item() if ious else 0.0

    def select_sam_masks(self, sam_masks, ts, H, W, device):
        """The mask bookkeeping of `_apply_segmentation` (ddim.py:739-903) for PRECOMPUTED candidate masks (the
        Grounded-SAM-2 producer itself is out of scope).  `sam_masks[i]` = the masks SAM would return for frame i, shape
        [n_i, H, W] (None / empty = no box detected).  Per frame, in order, with `pre_masks` starting at None (:391):
          * only frames with timestep <= 300 are touched (:592);
          * no detection -> previous masks, or nothing if there are none yet (:788-793);
          * IoU(new, previous) < 0.5 -> previous masks (:804-807);
          * masks are applied in order; one covering > 80 % of the frame RESETS what the earlier ones injected (:820-822).
        Returns (effective [f, H*W] float mask, frame mask index [f] with -1 = no injection)."""
        f = len(ts)
        eff = torch.zeros(f, H * W, dtype=torch.float32, device=device)
        midx = np.full((f,), -1, dtype=np.int32)
        pre = None
        for i in range(f):
            if float(ts[i]) > 300:
                continue
            cand = sam_masks[i] if i < len(sam_masks) else None
            if cand is not None:
                cand = torch.as_tensor(cand, device=device).float().reshape(-1, H, W)
            if cand is None or cand.shape[0] == 0:
                if pre is None:
                    continue                                   # returns (pred_x0, None): pre_masks stays None
                masks = pre
            else:
                masks = cand
                if pre is not None and self.calculate_iou(masks, pre) < 0.5:
                    masks = pre
            pre = masks
            cur = torch.zeros(H, W, dtype=torch.bool, device=device)
            for m in masks:
                if m.sum() > 0.8 * m.numel():
                    cur.zero_()                                # modified_pred_x0 = pred_x0 (:821)
                    continue
                cur |= m > 0.5
            eff[i] = cur.reshape(-1).float()
            midx[i] = i
        return eff, midx

    def step_tables(self, indices, ts_np, H, Fm):
        """Host-side tables of one `ddim_step` call (they depend on the window slot only, not on the data): coef [f][6] =
        {sqrt(a_t), sqrt(a_prev), sigma_t, sqrt(1-a_t), sqrt(1-a_prev-sigma^2), 2(1-t/1000)} evaluated in fp32 exactly as the
        reference's 0-dim tensors are (ddim.py:409-428), enh [f] (:582) and the mask frame consulted for each frame (:565-567
        incl. the clobbered loop variable, -1 = none; `Fm` = mask frames available)."""
        f32 = np.float32
        f = len(indices)
        coef = np.zeros((f, 6), dtype=np.float32)
        enh = np.ones((f,), dtype=np.float32)
        midx = np.full((f,), -1, dtype=np.int32)
        for i, index in enumerate(indices):
            coef[i, :5] = ddim_coef(self, index)                       # :415,562,418
            coef[i, 5] = f32(2) * (f32(1.0) - f32(ts_np[i]) / f32(1000.0))   # correction_strength :428
            enh[i] = 1.5 if ts_np[i] <= 300 else 1.0                   # :582
            mi = i
            if self.reference_index_quirk and i >= 1:
                mi = len(range(0, H, 4)) - 1                            # clobbered `i` (:477,502,533)
            if Fm > mi:                                                 # :565
                midx[i] = mi
        return coef, enh, midx

    @torch.no_grad()
    def ddim_step(self, sample, noise_pred, indices, cond_image, target, ts, gamma=0.5, use_self_attention=False,
                  davis_masks=None, noise=None, sam_masks=None, sam_masks_fn=None):
        """ddim.py:377-649.  Returns (x_prev, pred_x0); `self.momentum` persists across calls (:395-397).

        Mask semantics follow the reference bit for bit, quirk included: its plotting loops
        reuse the loop variable `i` (ddim.py:477,502,533), so for every frame i >= 1 the mask
        frame consulted at :565-567 is ceil(H/4)-1, not i (frame 0 uses mask frame 0).  Set
        `self.reference_index_quirk = False` for the per-frame mask the code evidently meant.
        Without `davis_masks` the reference calls Grounded-SAM-2 per frame (out of scope); pass what it would
        return as `sam_masks` (list over frames of [n,H,W] candidate masks) to get that branch's behaviour
        (`select_sam_masks`: t <= 300 only, IoU fallback, > 80 % reset, factor 2); with neither, no injection.
        `sam_masks_fn(pred_x0_frame [1,C,1,H,W], target, frame) -> [n,H,W] or None` is the mask PRODUCER interface (what
        `_apply_segmentation` does with Grounded-SAM-2, ddim.py:745-801): it is shown the momentum-corrected pred_x0 of every frame
        with t <= 300 (a first pass of the same kernel without injection and gamma = 0 yields it) and its answers go through the
        same bookkeeping as `sam_masks`."""
        if sam_masks_fn is not None and sam_masks is None and davis_masks is None:
            _, p0 = self.ddim_step(sample, noise_pred, indices, cond_image, target, ts, gamma=0.0, use_self_attention=True, noise=noise
                                   if noise is not None else torch.zeros_like(sample))
            ts_h = np.asarray(ts.detach().cpu()) if torch.is_tensor(ts) else np.asarray(ts)
            sam_masks = [sam_masks_fn(p0[:, :, [i]], target, i) if ts_h[i] <= 300 else None for i in range(sample.shape[2])]
        b, Cc, f, H, W = sample.shape
        device = sample.device
        sample, noise_pred = _f32c(sample), _f32c(noise_pred)
        if noise is None:
            noise = torch.randn(sample.shape, device=device)          # per-frame noise_like draws, :561
        noise = _f32c(noise)
        if not hasattr(self, 'momentum') or self.momentum.shape != sample.shape:
            self.momentum = torch.zeros_like(sample)                   # :395-397
        f32 = np.float32
        ts_np = np.asarray(ts.detach().cpu()) if torch.is_tensor(ts) else np.asarray(ts)
        Fm = int(davis_masks.shape[2]) if davis_masks is not None else 0
        coef, enh, midx = self.step_tables(indices, ts_np, H, Fm)
        x_prev, pred_x0 = torch.empty_like(sample), torch.empty_like(sample)
        coef_d = torch.from_numpy(coef).to(device)
        mask_d = cond_d = midx_d = enh_d = ws = None
        if davis_masks is None and sam_masks is not None and not use_self_attention:
            if b != 1:
                raise ValueError("the segmentation branch squeezes the batch axis (ddim.py:746-747): batch must be 1")
            eff, midx = self.select_sam_masks(sam_masks, ts_np, H, W, device)
            davis_masks = eff.reshape(1, 1, f, H, W)            # same injection kernel, other factor / frame selection
            Fm = f
            enh[:] = 2.0                                        # enhancement_factor = 2 (:847)
        if davis_masks is not None:
            mask_d = _f32c(davis_masks.to(device)).reshape(b, 1, Fm, H * W)
            cond_d = cond_image_rows(cond_image, Cc, H * W, device).expand(b, Cc, H * W).contiguous()      # :573-578
            midx_d = torch.from_numpy(midx).to(device)
            enh_d = torch.from_numpy(enh).to(device)
            ws = torch.empty(max(Fm, 1), dtype=torch.float32, device=device)
        _l.check(_l.load().moca_fifo_ddim_step_f32(
            _l.ptr(sample), _l.ptr(noise_pred), _l.ptr(noise), _l.ptr(self.momentum), _l.ptr(x_prev), _l.ptr(pred_x0),
            _l.ptr(coef_d), _l.ptr(mask_d), _l.ptr(cond_d), _l.ptr(midx_d), _l.ptr(enh_d), _l.ptr(ws),
            b, Cc, f, Fm, H * W, f32(self.beta), f32(1 - self.beta), f32(gamma), f32(1 - gamma), _st()),
            "moca_fifo_ddim_step_f32")
        return x_prev, pred_x0


class DPMSolverSampler(DDIMSampler):
    """DPM-Solver++(2M) (Lu et al., 2022: data prediction, multistep, midpoint form) on `DDIMSampler`'s integer timestep grid and its
    one-graph step: `sample`, `decode` and `sample_freeinit` with the parent's signatures and return shapes, every step
    `moca_base_ddim_step_f32` with MOCA_BASE_MULTISTEP over the tables of `fifo_graph.dpmpp_tables` -- replayed by `fifo_graph.DpmEngine`
    where `DpmEngine.supported` allows it, else host-issued through the same entry point (`_steps_host`): one kernel serves both.
    A trajectory over n schedule rows steps all but the identity rows at the clean end (`uniform` schedules have one, at timestep 0:
    one forward fewer than DDIM), first order on its first step and -- `lower_order_final` -- on its last, second order between them
    (`order` 1: first order throughout, which is DDIM at eta 0).  The solver is deterministic: `eta` other than 0, `noises=` and a
    temperature other than 1 are refused, nothing is drawn -- but for masked inpainting (`mask=` / `x0=` of `sample` and `decode`),
    whose blend in front of every stepped row draws q_sample's noise (`mask_noises=` fixes it); the identity rows at the clean end stay
    unstepped and unblended.  `p_sample_ddim`, `ddim_step`, `fifo_onestep`, `encode`,
    `stochastic_encode` are the parent's; FIFO / MoCA sampling refuses this sampler (`multistep`): diagonal denoising holds one frame
    per schedule level and moves each by one level per iteration, which ties the queue length to first-order steps."""
    multistep = True

    def __init__(self, model, order=2, lower_order_final=True, **kw):
        if isinstance(order, bool) or order not in (1, 2):
            raise ValueError(f"order = {order!r}: DPM-Solver++ multistep is built for orders 1 and 2")
        super().__init__(model, **kw)
        self.order, self.lower_order_final = int(order), bool(lower_order_final)

    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0., verbose=True):
        if ddim_eta != 0.:
            raise ValueError(f"eta = {ddim_eta}: DPM-Solver++ is a deterministic solver, its schedule has eta 0")
        super().make_schedule(ddim_num_steps, ddim_discretize=ddim_discretize, ddim_eta=0., verbose=verbose)

    @staticmethod
    def _refuse_draws(noises, temperature=1.):
        if noises is not None:
            raise ValueError("noises=: DPM-Solver++ draws nothing, there is no step noise to fix")
        if temperature != 1.:
            raise ValueError(f"temperature = {temperature}: DPM-Solver++ draws nothing, there is no step noise to scale")

    def _dpm_engine_for(self, img, cond, uc, scale, seed, n_rows, features_adapter=None, mask=None, x0=None):
        """the cached step graph (fifo_graph.DpmEngine) for this call, reset to a new trajectory; built when `DpmEngine.key` changes.  It
        shares the one-entry cache of the parent's engines."""
        return self._engines.get(DpmEngine.key(self, img, cond, uc, scale, features_adapter, n_rows, mask),
                                 lambda: DpmEngine(self.model, self, img, cond, uc, scale, seed=seed, features_adapter=features_adapter,
                                                   n_rows=n_rows, mask=mask, x0=x0),
                                 lambda eng: eng.reset(img, cond, uc, seed, features_adapter=features_adapter, mask=mask, x0=x0))

    def _on_graph(self, x, cond, uc, scale, use_graph, features_adapter):
        """-> (whether the call runs on `DpmEngine`, its unconditional branch: None without guidance)"""
        guided = uc is not None and scale != 1.0
        uc = uc if guided else None
        return bool(use_graph and (self.share_prefix or not guided)
                    and DpmEngine.supported(self.model, x, cond, uc, scale, features_adapter=features_adapter)), uc

    def _steps_host(self, x, cond, uc, scale, n_rows, features_adapter=None, mask=None, x0=None, mask_noises=None):
        """the host-issued trajectory over the first `n_rows` schedule rows: per stepped row [with a mask, `HostBlend` at the row's
        timestep,] `guidance_eps` + `cfg_combine`, then the engine's step launch on a private 32-byte state block, the device table and
        a history buffer (eps_u NULL: eps is combined)"""
        coef, t_table = dpmpp_tables(self, n_rows, self.order, self.lower_order_final)
        x = _f32c(x).clone()                                  # (the step kernel updates in place: the caller keeps x_T)
        dev = x.device
        state, coef_d, hist = state_block(0).to(dev), coef.to(dev), torch.empty_like(x)
        flags = _l.MOCA_BASE_MULTISTEP | (_l.MOCA_BASE_SCALE if self.use_scale else 0)
        unet_kwargs = {} if features_adapter is None else {"features_adapter": list(features_adapter)}
        blend = None if mask is None else HostBlend(self.model, x, mask, x0)
        for k in range(dpm_stepped_rows(coef)):
            if blend is not None:
                blend(x, int(t_table[n_rows - 1 - k]), None if mask_noises is None else mask_noises[k])
            ts = torch.full((x.shape[0],), int(t_table[n_rows - 1 - k]), device=dev, dtype=torch.long)
            e_t = _f32c(self._cfg_eps(x, ts, cond, uc, scale, **unet_kwargs))
            # (noise: required, not read)
            _l.check(_l.load().moca_base_ddim_step_f32(_l.ptr(state), _l.ptr(x), _l.ptr(e_t), None, _l.ptr(x), _l.ptr(hist), _l.ptr(coef_d),
                                                       n_rows, 1.0, flags, x.numel(), _st()), "moca_base_ddim_step_f32")
        return x

    def _run_steps(self, x, cond, uc, scale, n_steps, noises, use_graph, features_adapter=None, mask=None, x0=None, mask_noises=None):
        """the loop of `sample` and `decode`: the stepped rows among `ddim_timesteps[:n_steps]`, flipped, on `DpmEngine` where `use_graph`
        and `DpmEngine.supported` allow it, else host-issued; with `mask` / `x0` the blend in front of every stepped row"""
        self._refuse_draws(noises)
        if n_steps <= 0:
            return x
        graph, uc_g = self._on_graph(x, cond, uc, scale, use_graph, features_adapter)
        if graph:
            # (an unmasked trajectory draws nothing: seed 0; a masked one seeds its q-noise stream from the host generator)
            seed = 0 if mask is None or mask_noises is not None else int(torch.randint(0, 2 ** 62, (1,)).item())
            eng = self._dpm_engine_for(x, cond, uc_g, scale, seed, n_steps, features_adapter=features_adapter, mask=mask, x0=x0)
            for k in range(eng.n_stepped):
                eng.step(**({} if mask is None else {"mask_noise": None if mask_noises is None else mask_noises[k]}))
            return eng.latents().to(x.dtype)
        return self._steps_host(x, cond, uc, scale, n_steps, features_adapter=features_adapter, mask=mask, x0=x0,
                                mask_noises=mask_noises).to(x.dtype)

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, eta=0., x_T=None, verbose=False,
               unconditional_guidance_scale=1., unconditional_conditioning=None, latents_dir=None, noises=None,
               features_adapter=None, mask=None, x0=None, mask_noises=None, **kwargs):
        """`DDIMSampler.sample` with the solver's steps: S schedule rows, S - 1 forwards on a `uniform` schedule.  `mask` / `x0`: the
        parent's blend in front of every stepped row, `mask_noises[k]` fixing stepped row k's q-noise (`noises=` stays refused)"""
        self._refuse_draws(noises, kwargs.get("temperature", 1.))
        return super().sample(S, batch_size, shape, conditioning=conditioning, eta=eta, x_T=x_T, verbose=verbose,
                              unconditional_guidance_scale=unconditional_guidance_scale,
                              unconditional_conditioning=unconditional_conditioning, latents_dir=latents_dir, noises=None,
                              features_adapter=features_adapter, mask=mask, x0=x0, mask_noises=mask_noises, **kwargs)

    @torch.no_grad()
    def sample_freeinit(self, steps, batch_size, shape, LPF, conditioning=None, eta=0., x_T=None, z_rands=None, noises=None,
                        unconditional_guidance_scale=1., unconditional_conditioning=None, features_adapter=None, return_all=False,
                        verbose=False):
        """`DDIMSampler.sample_freeinit` with the solver's trajectories: on the step graph the whole run stays on ONE cached `DpmEngine`
        captured for steps[-1] rows (`set_schedule` where the step count changes, `reinit` between trajectories -- each starts on the
        first row of its table, so first order, whatever the history holds); elsewhere composed on the host from `freeinit_reinit`
        and `_steps_host`.  Only the fresh noise of a re-initialisation is drawn (`z_rands[k-1]` fixes it)."""
        from .freeinit import freeinit_reinit
        self._refuse_draws(noises)
        steps = [int(s) for s in steps]
        if not steps or max(steps) != steps[-1] or min(steps) < 1:
            raise ValueError(f"steps = {steps}: at least one trajectory, every one of 1 .. steps[-1] steps")
        if z_rands is not None and len(z_rands) != len(steps) - 1:
            raise ValueError(f"z_rands holds {len(z_rands)} tensors for {len(steps) - 1} re-initialisations")
        cond, uc, scale = conditioning, unconditional_conditioning, unconditional_guidance_scale
        self.make_schedule(ddim_num_steps=steps[-1], ddim_eta=eta, verbose=verbose)
        device = self.model.betas.device
        initial_noise = torch.randn((batch_size,) + tuple(shape), device=device) if x_T is None else x_T
        z_rand = lambda k: None if z_rands is None else z_rands[k - 1]
        every = []
        graph, uc_g = self._on_graph(initial_noise, cond, uc, scale, self.use_graph, features_adapter)
        if graph:
            eng = self._dpm_engine_for(initial_noise, cond, uc_g, scale, 0, steps[-1], features_adapter=features_adapter)
            for k, S in enumerate(steps):
                if S != eng.S - eng.it0:
                    self.make_schedule(ddim_num_steps=S, ddim_eta=eta, verbose=verbose)
                    eng.set_schedule(self)
                if k > 0:
                    seed = 0 if z_rand(k) is not None else int(torch.randint(0, 2 ** 62, (1,)).item())
                    eng.reinit(initial_noise, LPF, z_rand=z_rand(k), seed=seed)
                for _ in range(eng.n_stepped):
                    eng.step()
                if return_all:
                    every.append(eng.latents().to(initial_noise.dtype))
            x = every[-1] if return_all else eng.latents().to(initial_noise.dtype)
            return x, (every if return_all else None)
        x = initial_noise
        for k, S in enumerate(steps):
            if k > 0:
                zr = z_rand(k)
                x = freeinit_reinit(self.model, x, initial_noise, torch.randn_like(initial_noise, dtype=torch.float32) if zr is None else zr, LPF)
            self.make_schedule(ddim_num_steps=S, ddim_eta=eta, verbose=verbose)
            x = self._run_steps(x, cond, uc, scale, S, None, False, features_adapter=features_adapter)
            every.append(x)
        return x, (every if return_all else None)
