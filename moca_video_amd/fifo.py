"""Latent-queue side of the FIFO / MoCA loop (`scripts/evaluation/funcs.py`): `prepare_latents`
(:21-82), `shift_latents` (:86-99), `base_ddim_sampling` (:177-241), `v2v_ddim_sampling` (its start-from-a-clip sibling) and the window scheduling of
`fifo_ddim_sampling` (:243-373).  The queue stays resident in HBM; VAE decoding of emitted frames
(funcs.py:359-365) is outside the hot path: the loop hands each emitted latent to `emit`.
Noise is an optional explicit argument wherever the reference calls torch.randn*."""
from __future__ import annotations

import numpy as np
import torch

from .conditioning import refuse_concat, refuse_image_attention, refuse_long_window
from .fifo_graph import FifoEngine, fifo_windows, lookahead_schedule
from .freeinit import freeinit_steps, freq_mix_3d, get_freq_filter
from .sampler import DDIMSampler, DPMSolverSampler, noise_queue


def prepare_latents(args, input_path, sampler, model=None, data=None, initial_latents=None, noises=None):
    """funcs.py:21-82: frame j of the queue = sqrt(a_j) z[frame_idx] + sqrt(1-a_j) eps, frame_idx = max(0, j - (N - z.shape[2]));
    with lookahead the first f/2 frames all use a_0.  z = the cached base-sampling latents (`{N}.pt`), `initial_latents`, or --
    DAVIS mode, `data=(frames [b,3|4,t,H,W], masks)` -- the VAE encoding of the frames (`model.encode_first_stage_2DAE`)."""
    if data is not None:                                      # DAVIS branch, funcs.py:38-48
        frames, _masks = data
        frames = frames.to("cuda")
        if frames.shape[1] == 4:                              # RGBA -> RGB (:44-45)
            frames = frames[:, :3]
        initial_latents = model.encode_first_stage_2DAE(frames)
    elif initial_latents is None:
        initial_latents = torch.load(input_path + f"/{args.num_inference_steps}.pt")
    z = initial_latents.to("cuda", torch.float32).contiguous()
    tz = z.shape[2]
    n_look = args.video_length // 2 if args.lookahead_denoising else 0
    N = args.num_inference_steps
    # per queue frame: which base frame it starts from and its noise level (:55-77); the arithmetic over the latents is one kernel
    alphas = torch.as_tensor(np.asarray(sampler.ddim_alphas), dtype=torch.float32)
    return noise_queue(z, torch.cat([alphas[:1].expand(n_look), alphas[:N]]), [0] * n_look + [max(0, i - (N - tz)) for i in range(N)], noises)


def shift_latents(latents, davis_data=None, model=None, noise=None, anchor_noise=None):
    """funcs.py:86-118: dequeue frame 0, shift left, enqueue FreeInit-mixed noise.

    Prompt mode (`davis_data` None, :88-99): the FreeInit anchor is the dequeued frame.  Returns `latents`.
    DAVIS mode (`davis_data = (frames [b,3|4,t,H,W], masks [b,1,t,h,w])`, :101-118): the anchor is the VAE encoding
    (`model.encode_first_stage_2DAE`, a fresh posterior sample per call; `anchor_noise` [b,4,1,h,w] fixes the draw) of the
    LAST DAVIS frame, and the mask queue is shifted with its tail refilled from its own last frame.  Returns
    `(latents, (frames, masks))` like the reference."""
    if davis_data is None:
        anchor_frame = latents[:, :, 0].clone().unsqueeze(2)
    else:
        frames, masks = davis_data
        anchor_frame = frames[:, :, -1].clone().unsqueeze(2)
        if anchor_frame.shape[1] == 4:                        # RGBA -> RGB (:104-105)
            anchor_frame = anchor_frame[:, :3]
        anchor_frame = model.encode_first_stage_2DAE(anchor_frame.to(latents.device), noise=anchor_noise)
    latents[:, :, :-1] = latents[:, :, 1:].clone()
    new_noise = (torch.randn_like(latents[:, :, -1]) if noise is None else noise.to(latents.device, latents.dtype).reshape(latents[:, :, -1].shape)).unsqueeze(2)
    freq_filter = get_freq_filter(anchor_frame.shape, latents.device, "gaussian", 1, 0.25, 0.25)
    latents[:, :, -1] = freq_mix_3d(anchor_frame, new_noise, freq_filter).squeeze(2)
    if davis_data is None:
        return latents
    masks[:, :, :-1] = masks[:, :, 1:].clone()
    masks[:, :, -1] = masks[:, :, -1].clone()                 # :116 (the tail keeps the last DAVIS mask)
    return latents, (frames, masks)


def uncond_embedding(model, c_emb, uc_emb):
    """The unconditional context of funcs.py:199-208 / :268-270: `model.uncond_type == "empty_seq"` (the YAML's value) is
    the text encoding of the EMPTY PROMPT -- it needs the text encoder, so the caller must pass it (`uc_emb`, e.g.
    `embed_text("")`); only `"zero_embed"` is zeros.  Passing nothing under "empty_seq" raises instead of silently
    sampling with a different unconditional branch than the reference."""
    if uc_emb is not None:
        return uc_emb
    utype = getattr(model, "uncond_type", "empty_seq")
    if utype == "zero_embed":
        return torch.zeros_like(c_emb)
    if utype == "empty_seq":
        if getattr(model, "cond_stage_model", None) is not None and hasattr(model, "empty_prompt_tokens"):
            return model.get_learned_conditioning(model.empty_prompt_tokens.expand(c_emb.shape[0], -1))
        raise ValueError('uncond_type == "empty_seq": classifier-free guidance needs the text encoding of the empty prompt; '
                         'pass uc_emb=embed_text("") (funcs.py:199-203)')
    raise NotImplementedError(f"uncond_type {utype!r}")


def base_uncond(model, cond, batch, cfg_scale, uc_emb=None):
    """the unconditional branch of funcs.py:197-216 (None without guidance): `model.uncond_type`'s context -- for an image-conditioned
    model followed by the image tokens of a zero image (:207-210) -- in a copy of `cond` that replaces `c_crossattn` only (:211-214)"""
    return uncond_like(model, cond, cfg_scale, uc_emb, image_tokens_for=batch)


def uncond_like(model, cond, cfg_scale, uc_emb=None, image_tokens_for=None):
    """None without guidance, else `cond` with `model.uncond_type`'s context (funcs.py:199-206, :268-270) in place of `c_crossattn`
    (a copy of the dict that replaces that key only, :211-214; the bare context for a bare `cond`).  `image_tokens_for` = batch: an
    image-conditioned model appends the image tokens of a zero image (:207-210), which `base_ddim_sampling` does and the FIFO loop
    does not."""
    if cfg_scale == 1.0:
        return None
    uc_emb = uncond_embedding(model, cond["c_crossattn"][0] if isinstance(cond, dict) else cond, uc_emb)
    if image_tokens_for is not None and hasattr(model, "embedder"):
        uc_img = model.get_image_embeds(torch.zeros(image_tokens_for, 3, 224, 224, device=model.device))
        uc_emb = torch.cat([uc_emb, uc_img], dim=1)
    return dict(cond, c_crossattn=[uc_emb]) if isinstance(cond, dict) else uc_emb


def base_ddim_sampling(model, cond, noise_shape, ddim_steps=50, ddim_eta=1.0, cfg_scale=1.0, uc_emb=None,
                       latents_dir=None, x_T=None, noises=None, use_graph=True):
    """funcs.py:177-241: returns (batch_images, ddim_sampler, samples) like the reference; batch_images is the VAE
    decode of the samples (:239) when the model was built with `first_stage_config`, else None.  `uc_emb` replaces
    model.get_learned_conditioning([""]) (the text encoder is out of scope)."""
    sampler = DDIMSampler(model)
    sampler.use_graph = use_graph            # one hipGraph per DDIM step (fifo_graph.BaseEngine) vs host-issued p_sample_ddim
    uc = base_uncond(model, cond, noise_shape[0], cfg_scale, uc_emb)
    samples, _ = sampler.sample(S=ddim_steps, conditioning=cond, batch_size=noise_shape[0], shape=noise_shape[1:],
                                verbose=False, unconditional_guidance_scale=cfg_scale, unconditional_conditioning=uc,
                                eta=ddim_eta, x_T=x_T, latents_dir=latents_dir, noises=noises)
    sampler.release()                        # the step graph's buffers: the FIFO stage that follows builds its own plan
    images = model.decode_first_stage_2DAE(samples) if getattr(model, "first_stage_model", None) is not None else None
    return images, sampler, samples


def freeinit_ddim_sampling(model, cond, noise_shape, ddim_steps=50, ddim_eta=1.0, cfg_scale=1.0, uc_emb=None, num_iters=5,
                           filter_type="butterworth", n=4, d_s=0.25, d_t=0.25, use_fast_sampling=False, x_T=None, z_rands=None,
                           noises=None, use_graph=True, return_all=False):
    """FreeInit (Wu et al., 2023) on `base_ddim_sampling`: sample, re-noise the result to t = num_timesteps - 1 with the INITIAL noise,
    keep its low spatio-temporal frequencies (`get_freq_filter(noise_shape, filter_type, n, d_s, d_t)`) and take the high ones from
    fresh noise (`freq_mix_3d`), sample again -- `num_iters` trajectories in all (`DDIMSampler.sample_freeinit`).  Every trajectory takes
    `ddim_steps` steps, or with `use_fast_sampling` `freeinit_steps`' coarse-to-fine counts.  num_iters = 1 is `base_ddim_sampling`.
    `x_T` fixes the initial noise, `z_rands[k-1]` the fresh noise of trajectory k >= 1, `noises[k][i]` the draw of its step i.
    Returns (images, sampler, samples) like `base_ddim_sampling` (the decode of the last trajectory); with `return_all`, `samples` is
    the list of every trajectory's latents."""
    steps = freeinit_steps(ddim_steps, num_iters, use_fast_sampling)
    if len(noise_shape) != 5:
        raise ValueError(f"noise_shape = {tuple(noise_shape)}: FreeInit filters over (T, H, W) of [B, C, T, H, W] latents")
    if z_rands is not None and len(z_rands) != num_iters - 1:
        raise ValueError(f"z_rands holds {len(z_rands)} tensors for {num_iters - 1} re-initialisations")
    if noises is not None and len(noises) != num_iters:
        raise ValueError(f"noises holds {len(noises)} lists for {num_iters} iterations")
    LPF = get_freq_filter(tuple(noise_shape), model.device, filter_type, n, d_s, d_t)
    sampler = DDIMSampler(model)
    sampler.use_graph = use_graph
    uc = base_uncond(model, cond, noise_shape[0], cfg_scale, uc_emb)
    last, every = sampler.sample_freeinit(steps, noise_shape[0], tuple(noise_shape[1:]), LPF, conditioning=cond, eta=ddim_eta, x_T=x_T,
                                          z_rands=z_rands, noises=noises, unconditional_guidance_scale=cfg_scale,
                                          unconditional_conditioning=uc, return_all=return_all)
    sampler.release()
    images = model.decode_first_stage_2DAE(last) if getattr(model, "first_stage_model", None) is not None else None
    return images, sampler, (every if return_all else last)


def v2v_ddim_sampling(model, cond, latents=None, frames=None, ddim_steps=50, t_start=25, ddim_eta=1.0, cfg_scale=1.0, uc_emb=None,
                      noise=None, noises=None, use_graph=True):
    """Video-to-video: noise a clip's latents to schedule index `t_start` (`DDIMSampler.stochastic_encode`, ddim.py:652-671) and
    denoise them under `cond` for t_start steps (`DDIMSampler.decode`, :674-692) -- the upstream img2img convention, so
    1 <= t_start <= ddim_steps - 1.  Exactly one of `latents` [B,4,T,h,w] and `frames` [B,3,T,H,W] (VAE-encoded first,
    `encode_first_stage_2DAE`).  The unconditional branch is `base_ddim_sampling`'s.  `noise` fixes the encode draw, `noises[i]` the
    draw of decode step i.  Returns (images, sampler, samples) like `base_ddim_sampling`."""
    if (latents is None) == (frames is None):
        raise ValueError("v2v_ddim_sampling wants exactly one of latents= and frames=")
    if not 1 <= int(t_start) <= int(ddim_steps) - 1:
        raise ValueError(f"t_start = {t_start}: the clip is encoded at schedule index t_start and decoded over t_start steps, "
                         f"so 1 <= t_start <= ddim_steps - 1 = {int(ddim_steps) - 1}")
    t_start = int(t_start)
    if frames is not None:
        latents = model.encode_first_stage_2DAE(frames.to(model.device))
    x0 = latents.to(model.device)
    sampler = DDIMSampler(model)
    sampler.use_graph = use_graph
    sampler.make_schedule(ddim_num_steps=ddim_steps, ddim_eta=ddim_eta, verbose=False)
    uc = base_uncond(model, cond, x0.shape[0], cfg_scale, uc_emb)
    t = torch.full((x0.shape[0],), t_start, dtype=torch.long)
    x_enc = sampler.stochastic_encode(x0, t, noise=noise)
    samples = sampler.decode(x_enc, cond, t_start, unconditional_guidance_scale=cfg_scale, unconditional_conditioning=uc, noises=noises)
    sampler.release()
    images = model.decode_first_stage_2DAE(samples) if getattr(model, "first_stage_model", None) is not None else None
    return images, sampler, samples


def dpm_solver_sampling(model, cond, noise_shape, steps=20, order=2, cfg_scale=1.0, uc_emb=None, x_T=None, use_graph=True,
                        lower_order_final=True):
    """`base_ddim_sampling` with DPM-Solver++(2M) (`DPMSolverSampler`) in place of DDIM: `steps` schedule rows on the same `uniform`
    grid, steps - 1 UNet forwards (the row at timestep 0 is an identity), deterministic -- `x_T` is the only draw.  Returns
    (images, sampler, samples) like `base_ddim_sampling`."""
    sampler = DPMSolverSampler(model, order=order, lower_order_final=lower_order_final)
    sampler.use_graph = use_graph
    uc = base_uncond(model, cond, noise_shape[0], cfg_scale, uc_emb)
    samples, _ = sampler.sample(S=steps, conditioning=cond, batch_size=noise_shape[0], shape=noise_shape[1:], verbose=False,
                                unconditional_guidance_scale=cfg_scale, unconditional_conditioning=uc, x_T=x_T)
    sampler.release()
    images = model.decode_first_stage_2DAE(samples) if getattr(model, "first_stage_model", None) is not None else None
    return images, sampler, samples


def v2v_dpm_solver_sampling(model, cond, latents=None, frames=None, steps=20, t_start=10, order=2, cfg_scale=1.0, uc_emb=None, noise=None,
                            use_graph=True, lower_order_final=True):
    """`v2v_ddim_sampling` with DPM-Solver++(2M): the clip's latents noised to schedule index `t_start` (`stochastic_encode`; `noise`
    fixes that draw, the only one), then the multistep `decode` over the first t_start schedule rows.  1 <= t_start <= steps - 1.
    Returns (images, sampler, samples) like `base_ddim_sampling`."""
    if (latents is None) == (frames is None):
        raise ValueError("v2v_dpm_solver_sampling wants exactly one of latents= and frames=")
    if not 1 <= int(t_start) <= int(steps) - 1:
        raise ValueError(f"t_start = {t_start}: the clip is encoded at schedule index t_start and decoded over t_start rows, "
                         f"so 1 <= t_start <= steps - 1 = {int(steps) - 1}")
    t_start = int(t_start)
    if frames is not None:
        latents = model.encode_first_stage_2DAE(frames.to(model.device))
    x0 = latents.to(model.device)
    sampler = DPMSolverSampler(model, order=order, lower_order_final=lower_order_final)
    sampler.use_graph = use_graph
    sampler.make_schedule(ddim_num_steps=steps, verbose=False)
    uc = base_uncond(model, cond, x0.shape[0], cfg_scale, uc_emb)
    x_enc = sampler.stochastic_encode(x0, torch.full((x0.shape[0],), t_start, dtype=torch.long), noise=noise)
    samples = sampler.decode(x_enc, cond, t_start, unconditional_guidance_scale=cfg_scale, unconditional_conditioning=uc)
    sampler.release()
    images = model.decode_first_stage_2DAE(samples) if getattr(model, "first_stage_model", None) is not None else None
    return images, sampler, samples


def latent_mask(mask, latent_shape, factor=8):
    """the inpainting mask at latent resolution.  A mask whose last two dims are the latents' goes through as it is; one at pixel
    resolution [.., factor h, factor w] is reduced once, on the host side of the sampler: a latent cell is kept (1) only if ALL of its
    factor x factor pixels are kept -- a min-pool, so a cell the caller wants partly regenerated is regenerated"""
    h, w = int(latent_shape[-2]), int(latent_shape[-1])
    if mask.dim() < 2:
        raise ValueError(f"mask {tuple(mask.shape)} has no (H, W) dims")
    if tuple(mask.shape[-2:]) == (h, w):
        return mask
    if tuple(mask.shape[-2:]) != (factor * h, factor * w):
        raise ValueError(f"mask {tuple(mask.shape)}: its last two dims are neither the latents' {(h, w)} nor the pixels' {(factor * h, factor * w)}")
    lead = tuple(mask.shape[:-2])
    return mask.to(torch.float32).reshape(lead + (h, factor, w, factor)).amin(dim=(-3, -1))


def _inpaint_sampling(sampler, model, cond, mask, latents, frames, n_rows, cfg_scale, uc_emb, x_T, t_start, paste_back, noise, sample_kw,
                      decode_kw):
    """the common body of `inpaint_ddim_sampling` and `inpaint_dpm_solver_sampling` on a sampler whose schedule is made"""
    from .sampler import HostBlend, check_inpaint
    if (latents is None) == (frames is None):
        raise ValueError("inpainting wants exactly one of latents= and frames=: the clip whose masked region is kept")
    if frames is not None:
        latents = model.encode_first_stage_2DAE(frames.to(model.device))
    x0 = latents.to(model.device)
    mask = latent_mask(mask.to(model.device), x0.shape)
    check_inpaint(x0.shape, mask, x0)
    if t_start is not None and not 1 <= int(t_start) <= int(n_rows) - 1:
        raise ValueError(f"t_start = {t_start}: the clip is encoded at schedule index t_start and decoded over t_start rows, "
                         f"so 1 <= t_start <= {int(n_rows) - 1}")
    uc = base_uncond(model, cond, x0.shape[0], cfg_scale, uc_emb)
    if t_start is None:                                       # from noise: `sample`
        samples, _ = sampler.sample(S=n_rows, conditioning=cond, batch_size=x0.shape[0], shape=tuple(x0.shape[1:]), verbose=False,
                                    unconditional_guidance_scale=cfg_scale, unconditional_conditioning=uc, x_T=x_T, mask=mask, x0=x0,
                                    **sample_kw)
    else:                                                     # from the clip itself, noised to row t_start: the v2v path
        t_start = int(t_start)
        x_enc = sampler.stochastic_encode(x0, torch.full((x0.shape[0],), t_start, dtype=torch.long), noise=noise)
        samples = sampler.decode(x_enc, cond, t_start, unconditional_guidance_scale=cfg_scale, unconditional_conditioning=uc, mask=mask,
                                 x0=x0, **decode_kw)
    sampler.release()
    if paste_back:
        samples = HostBlend(model, samples, mask, x0).paste(samples.to(torch.float32).contiguous().clone())
    images = model.decode_first_stage_2DAE(samples) if getattr(model, "first_stage_model", None) is not None else None
    return images, sampler, samples


def inpaint_ddim_sampling(model, cond, mask, latents=None, frames=None, ddim_steps=50, ddim_eta=0., cfg_scale=1.0, uc_emb=None, x_T=None,
                          t_start=None, paste_back=True, use_graph=True, noise=None, noises=None, mask_noises=None):
    """Masked inpainting at DDIM speed: regenerate a clip where `mask == 0` and keep it where `mask == 1`, in `ddim_steps` forwards on
    the one-graph step (`DDIMSampler.sample` / `decode` with `mask=` / `x0=`: upstream's blend in front of every step).  A mask over
    frames continues a clip or fills in between kept frames; a mask over pixels inpaints.  Exactly one of `latents` [B,4,T,h,w] and
    `frames` [B,3,T,H,W] (VAE-encoded first, as in `v2v_ddim_sampling`) is the clip.  `mask` broadcasts against the latents, at latent
    resolution or at pixel resolution [.., 8h, 8w] (`latent_mask`: a latent cell is kept only if all of its 64 pixels are).
    `t_start` None: from noise (`x_T` fixes it) over the whole schedule; `t_start` = k: the clip noised to schedule row k
    (`stochastic_encode`, `noise` fixes that draw) and decoded over k rows, the video-to-video path, 1 <= k <= ddim_steps - 1.
    The sampler blends before every step and not behind the last, so its kept region is one DDIM step away from the clip;
    `paste_back` finishes with one launch of the same kernel on the clean row: the kept region of the returned latents then equals the
    clip's bit for bit.  `noises[i]` / `mask_noises[i]` fix step i's two draws.  Returns (images, sampler, samples) like
    `base_ddim_sampling`."""
    sampler = DDIMSampler(model)
    sampler.use_graph = use_graph
    sampler.make_schedule(ddim_num_steps=ddim_steps, ddim_eta=ddim_eta, verbose=False)
    draws = dict(noises=noises, mask_noises=mask_noises)
    return _inpaint_sampling(sampler, model, cond, mask, latents, frames, ddim_steps, cfg_scale, uc_emb, x_T, t_start, paste_back, noise,
                             dict(draws, eta=ddim_eta), draws)


def inpaint_dpm_solver_sampling(model, cond, mask, latents=None, frames=None, steps=20, order=2, cfg_scale=1.0, uc_emb=None, x_T=None,
                                t_start=None, paste_back=True, use_graph=True, lower_order_final=True, noise=None, mask_noises=None):
    """`inpaint_ddim_sampling` with DPM-Solver++(2M) (`DPMSolverSampler`): `steps` schedule rows, the blend in front of every stepped
    row (the identity rows at the clean end stay unstepped and unblended), q_sample's noise the solver's only draw
    (`mask_noises[k]` fixes stepped row k's).  Returns (images, sampler, samples) like `base_ddim_sampling`."""
    sampler = DPMSolverSampler(model, order=order, lower_order_final=lower_order_final)
    sampler.use_graph = use_graph
    sampler.make_schedule(ddim_num_steps=steps, verbose=False)
    draws = dict(mask_noises=mask_noises)
    return _inpaint_sampling(sampler, model, cond, mask, latents, frames, steps, cfg_scale, uc_emb, x_T, t_start, paste_back, noise,
                             draws, draws)


def refuse_multistep(sampler):
    """the FIFO loops take `DDIMSampler`'s first-order step only"""
    if getattr(sampler, "multistep", False):
        raise NotImplementedError(f"{type(sampler).__name__} cannot drive FIFO / MoCA sampling: diagonal denoising holds one queue frame per "
                                  "schedule level and moves every frame by one level per iteration, which ties the queue length to "
                                  "first-order steps; a multistep solver would need a history per frame and another queue")


def v2v_invert_sampling(model, cond, latents=None, frames=None, ddim_steps=50, t_start=25, ddim_eta=0.0, cfg_scale=1.0, uc_emb=None,
                        src_cond=None, src_cfg_scale=1.0, noises=None, use_graph=True):
    """`v2v_ddim_sampling` with the clip taken to schedule index `t_start` by its own deterministic DDIM inversion
    (`DDIMSampler.encode`) instead of by noise (`stochastic_encode`): t_start inversion steps under `src_cond` (default: `cond`) with
    guidance `src_cfg_scale` -- the state is then at level ddim_alphas[t_start - 1], where `decode(x, cond, t_start)` starts -- and
    t_start denoising steps under `cond` with guidance `cfg_scale`.  With src_cond = cond, eta 0 (the default here) and no guidance
    the two halves are a round trip; a new `cond` edits the clip and keeps what the inversion kept of it.  There is no encode draw, so
    no `noise=` (and `t_start` may be the whole schedule); `noises[i]` fixes the draw of decode step i when eta > 0.  Its own function
    beside `v2v_ddim_sampling`, whose parameter list is pinned.  Returns (images, sampler, samples) like `base_ddim_sampling`."""
    if (latents is None) == (frames is None):
        raise ValueError("v2v_invert_sampling wants exactly one of latents= and frames=")
    if not 1 <= int(t_start) <= int(ddim_steps):
        raise ValueError(f"t_start = {t_start}: the clip is inverted over t_start steps and decoded over as many, "
                         f"so 1 <= t_start <= ddim_steps = {int(ddim_steps)}")
    t_start = int(t_start)
    if frames is not None:
        latents = model.encode_first_stage_2DAE(frames.to(model.device))
    x0 = latents.to(model.device)
    sampler = DDIMSampler(model)
    sampler.use_graph = use_graph
    sampler.make_schedule(ddim_num_steps=ddim_steps, ddim_eta=ddim_eta, verbose=False)
    src_cond = cond if src_cond is None else src_cond
    x_enc, _ = sampler.encode(x0, src_cond, t_start, unconditional_guidance_scale=src_cfg_scale,
                              unconditional_conditioning=base_uncond(model, src_cond, x0.shape[0], src_cfg_scale, uc_emb))
    uc = base_uncond(model, cond, x0.shape[0], cfg_scale, uc_emb)
    samples = sampler.decode(x_enc, cond, t_start, unconditional_guidance_scale=cfg_scale, unconditional_conditioning=uc, noises=noises)
    sampler.release()
    images = model.decode_first_stage_2DAE(samples) if getattr(model, "first_stage_model", None) is not None else None
    return images, sampler, samples


def fifo_ddim_sampling(args, model, conditioning, noise_shape, ddim_sampler, cfg_scale=1.0, uc_emb=None,
                       latents=None, latents_dir=None, conditioned_image=None, masks=None, gamma=0.5, emit=None,
                       n_iterations=None, batch_windows=True, noises=None, shift_noises=None, decode=False, decode_batch=8,
                       davis_data=None, anchor_noises=None, sam_masks=None, sam_masks_fn=None, targets=None, use_graph=True,
                       seed=None, sam_capacity=None, **kwargs):
    """funcs.py:243-373: returns the list of emitted latent frames [B,4,1,h,w]; with decode=True (and a model built with
    `first_stage_config`) the list of decoded frames [B,3,1,8h,8w] instead -- `model.decode_first_stage_2DAE` of funcs.py:360,
    run on `decode_batch` emitted frames at a time rather than once per iteration.

    Injection masks, as in the reference: with `davis_data = (frames, masks)` (DAVIS-video mode) the masks come from it and every
    queue shift takes the DAVIS branch of `shift_latents` (funcs.py:101-118,368-369); `masks` [B,1,Q,h,w] handed in directly play
    the same role (`davis_masks` of ddim_step: factor 1.5 / 1.0, every timestep).  WITHOUT either the reference's `ddim_step`
    takes its segmentation branch (ddim.py:592-606: only frames with t <= 300, IoU fallback, > 80 % reset, factor 2) and asks
    Grounded-SAM-2 for masks -- out of scope here, so they come in as `sam_masks[i][w]` (iteration i, window w in the reference's
    call order: the list over frames of [n,h,w] candidate masks; or a callable (i, w) -> that list) or from `sam_masks_fn(pred_x0_frame, targets, frame) -> [n,h,w]`
    (see DDIMSampler.ddim_step); with neither, nothing is injected.  Candidate LISTS run inside the iteration graph
    (`moca_sam_select_masks_f32`; `sam_capacity` = the most candidate masks one iteration may hold, default: counted when
    `sam_masks` is a list, else 4 per window frame); a producer CALLBACK needs pred_x0 on the host frame by frame and stays on the
    host-driven loop.

    batch_windows=True evaluates the 2n windows of an iteration as one batched UNet launch; with `use_graph` (and a
    call `FifoEngine.supported` accepts) the WHOLE iteration -- gather, UNet, guidance, ddim_step of all windows, write-back,
    emission, FreeInit mix, shift -- is one hipGraph on a device-resident ring queue (fifo_graph.py) and the host never
    synchronises inside the loop; `latents` / `masks` are updated in place at the end like the reference's tensors.
    `noises[i][w]` / `shift_noises[i]` optionally fix the per-window DDIM noise and the enqueued noise (else: device Philox
    stream keyed by `seed` on the graph path, torch.randn on the host path).

    `context_at(i)` (keyword; the hook of `fifo_ddim_sampling_multiprompts`): called at the top of iteration i; None keeps the
    conditional context, a tensor [1,L,D] replaces it from this iteration on (same L; on the graph path `FifoEngine.set_context`)."""
    context_at = kwargs.pop("context_at", None)
    kwargs.update({"clean_cond": True})
    refuse_multistep(ddim_sampler)
    refuse_long_window(args)
    refuse_image_attention(model)
    refuse_concat(model, conditioning)
    cond = conditioning
    uc = uncond_like(model, cond, cfg_scale, uc_emb)       # :268-270
    if davis_data is not None:
        davis_data = (davis_data[0].to(model.device), davis_data[1].to(model.device))     # :296-300
        masks = davis_data[1]
    if latents is None:
        latents = prepare_latents(args, latents_dir, ddim_sampler, model=model, data=davis_data)
    f = args.video_length
    timesteps, indices = lookahead_schedule(ddim_sampler, args)
    total = args.new_video_length + args.num_inference_steps - f if n_iterations is None else n_iterations
    frames, pending = [], []

    sam_in_graph = sam_masks is not None and masks is None                      # (with masks the DAVIS branch wins, ddim.py:565)
    if (batch_windows and use_graph and FifoEngine.supported(model, cond, latents, davis_data=davis_data, sam_masks_fn=sam_masks_fn) and
            (masks is None or masks.shape[2] == latents.shape[2])):
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())                # follows torch.manual_seed like the randn draws it replaces
        moments = None
        if davis_data is not None:                       # :101-108: the anchor frame never changes -> its posterior moments, once
            last = davis_data[0][:, :, -1]
            if last.shape[1] == 4:
                last = last[:, :3]
            moments = model.first_stage_model.encode(last.to(latents.device)).parameters
        sam_of = (lambda i: None) if not sam_in_graph else \
            (lambda i: [sam_masks(i, w) for w in range(len(list(fifo_windows(args))))]) if callable(sam_masks) else (lambda i: sam_masks[i])
        if sam_in_graph and sam_capacity is None:
            n_wf = len(list(fifo_windows(args))) * f
            # (a list: the exact maximum over the iterations, an iteration / window / frame entry may be None; a callable: a guess of 4
            #  candidate masks per window frame -- pass `sam_capacity` explicitly when the producer can return more: an iteration that
            #  exceeds the pool raises ValueError from FifoEngine._upload_sam, after earlier frames have been emitted)
            sam_capacity = 4 * n_wf if callable(sam_masks) else max(
                [1] + [sum(0 if c is None else int(torch.as_tensor(c).reshape(-1, latents.shape[-2], latents.shape[-1]).shape[0])
                           for cw in it if cw is not None for c in cw) for it in sam_masks[:total] if it is not None])
        eng = FifoEngine(args, model, ddim_sampler, cond, uc, cfg_scale, latents, conditioned_image=conditioned_image, masks=masks,
                         n_slots=decode_batch if decode else max(total, 1), seed=seed, anchor_moments=moments,
                         scale_factor=getattr(model, "scale_factor", 1.0), sam_capacity=sam_capacity if sam_in_graph else 0)
        try:
            for i in range(total):
                ctx = None if context_at is None else context_at(i)
                if ctx is not None:
                    eng.set_context(ctx)
                sm = sam_of(i)
                if noises is not None or shift_noises is not None or anchor_noises is not None:
                    nz = noises[i] if noises is not None else [torch.randn(noise_shape, device=latents.device) for _ in eng.wins]
                    sn = shift_noises[i] if shift_noises is not None else torch.randn_like(latents[:, :, -1])
                    an = None
                    if moments is not None:
                        an = anchor_noises[i] if anchor_noises is not None else torch.randn_like(latents[:, :, -1])
                    eng.step(noise=nz, shift_noise=sn, anchor_noise=an, sam_masks=sm)
                else:
                    eng.step(sam_masks=sm)
                if decode and ((i + 1) % decode_batch == 0 or i + 1 == total):
                    i0 = (i // decode_batch) * decode_batch
                    img = model.decode_first_stage_2DAE(eng.emitted_frames(i0, i + 1))
                    frames.extend(img[:, :, [k]] for k in range(img.shape[2]))
            if not decode and total > 0:
                z = eng.emitted_frames(0, total)
                frames = [z[:, :, [k]].clone() if emit is None else emit(z[:, :, [k]].clone()) for k in range(total)]
            latents.copy_(eng.latents().to(latents.dtype))
            if masks is not None:
                masks.copy_(eng.mask_queue().to(masks.dtype))
        finally:
            eng.close()
        return frames

    for i in range(total):
        ctx = None if context_at is None else context_at(i)
        if ctx is not None:
            cond = dict(cond, c_crossattn=[ctx])
        wins = list(fifo_windows(args))
        eps_list = None
        if batch_windows:
            # N2: all windows of this iteration as one batched UNet launch (they are independent, see unet_windows)
            eps_list = ddim_sampler.unet_windows([latents[:, :, s0:e0].clone() for s0, _, e0 in wins], cond,
                                                 [timesteps[s0:e0] for s0, _, e0 in wins],
                                                 unconditional_guidance_scale=cfg_scale, unconditional_conditioning=uc, **kwargs)
        for wi, (start, mid, end) in enumerate(wins):
            t, idx = timesteps[start:end], indices[start:end]
            input_latents = latents[:, :, start:end].clone()
            input_masks = masks[:, :, start:end].clone() if masks is not None else None
            noise = None if noises is None else noises[i][wi]
            sam = dict(sam_masks=None if sam_masks is None else (sam_masks(i, wi) if callable(sam_masks) else sam_masks[i][wi]),
                       sam_masks_fn=sam_masks_fn)
            if eps_list is not None:
                ts_t = torch.as_tensor(np.asarray(t).copy(), device=latents.device).to(torch.long)
                output_latents, _ = ddim_sampler.ddim_step(input_latents, eps_list[wi], idx, conditioned_image, targets, ts_t,
                                                           davis_masks=input_masks, noise=noise, **sam)
            else:
                output_latents, _ = ddim_sampler.fifo_onestep(cond=cond, shape=noise_shape, latents=input_latents, timesteps=t,
                                                              indices=idx, unconditional_guidance_scale=cfg_scale,
                                                              unconditional_conditioning=uc, cond_image=conditioned_image,
                                                              target=targets, davis_masks=input_masks, noise=noise, **sam, **kwargs)
            if args.lookahead_denoising:
                latents[:, :, mid:end] = output_latents[:, :, -(f // 2):]
            else:
                latents[:, :, start:end] = output_latents
        first = f // 2 if args.lookahead_denoising else 0
        frame = latents[:, :, [first]].clone()
        if decode:
            pending.append(frame)
            if len(pending) == decode_batch:
                frames.extend(decode_frames(model, pending))
                pending = []
        else:
            frames.append(frame if emit is None else emit(frame))
        sn = None if shift_noises is None else shift_noises[i]
        if davis_data is not None:                                                  # :367-369
            latents, davis_data = shift_latents(latents, davis_data, model, noise=sn,
                                                anchor_noise=None if anchor_noises is None else anchor_noises[i])
        else:
            latents = shift_latents(latents, noise=sn)
            if masks is not None:            # masks handed in directly (prompt mode + precomputed masks): keep them aligned
                masks[:, :, :-1] = masks[:, :, 1:].clone()
    if pending:
        frames.extend(decode_frames(model, pending))
    return frames


def multiprompt_segments(args, multiprompts, n_iterations=None):
    """funcs.py:379,420-427: the prompt segment j of every outer iteration of `fifo_ddim_sampling_multiprompts`.  `multiprompts[-1]`
    holds the comma-separated frame count of each prompt, prompt_lengths = their cumsum; the loop runs prompt_lengths[-1] + S - f
    iterations (`n_iterations`: the trange cut) and at the top of iteration i moves j by at most one,
    `if i - (S - f) >= prompt_lengths[j]: j += 1` -- a segment of 0 frames still lasts one iteration and the first S - f iterations
    stay on prompt 0, exactly as in the reference.  ValueError where the reference would index past its last prompt."""
    lengths = np.array([int(c) for c in multiprompts[-1].split(",")]).cumsum()
    if len(lengths) != len(multiprompts) - 1:
        raise ValueError(f"{len(lengths)} frame counts ({multiprompts[-1]!r}) for {len(multiprompts) - 1} prompts")
    warm = args.num_inference_steps - args.video_length
    total = int(lengths[-1]) + warm if n_iterations is None else int(n_iterations)
    seg, j = [], 0
    for i in range(total):
        if i - warm >= lengths[j]:
            j += 1
            if j == len(lengths):
                raise ValueError(f"iteration {i} runs past the last prompt (prompt_lengths {lengths.tolist()})")
        seg.append(j)
    return seg


def fifo_ddim_sampling_multiprompts(args, model, conditioning, noise_shape, ddim_sampler, multiprompts, cfg_scale=1.0,
                                    output_dir=None, latents_dir=None, save_frames=False, embeds=None, uc_emb=None, latents=None,
                                    noises=None, shift_noises=None, seed=None, decode=False, decode_batch=8, n_iterations=None,
                                    batch_windows=True, use_graph=True, conditioned_image=None, targets=None, sam_masks=None,
                                    sam_masks_fn=None, sam_capacity=None, emit=None, **kwargs):
    """funcs.py:375-468: one long video whose prompt changes over time.  `multiprompts` = [prompt_0, ..., prompt_n-1, "c_0,...,c_n-1"]
    (frame counts); the prompt of every iteration follows `multiprompt_segments`, and all windows of an iteration use that ONE
    prompt's context (77 tokens, not MoCA's two-prompt 154).  Returns what `fifo_ddim_sampling` returns, whose loop this is: on the
    one-graph path a switch is `FifoEngine.set_context` between two replays (no new plan, no capture), on the host-driven path the
    next iteration's conditioning.  `save_frames` (needs `decode=True`) writes `output_dir/fifo/{i}.png` like funcs.py:455-459.

    embeds: the per-prompt contexts [1,77,D] (the prompt strings then only name the segments); without them the model's text
    encoder embeds each prompt string (`model.get_learned_conditioning(prompt)`, funcs.py:382).  uc_emb: the unconditional
    context, which here is the EMPTY PROMPT whatever `model.uncond_type` says (funcs.py:398-399); needed when the model has no text
    encoder.  Queue: `latents`, else `prepare_latents` in prompt mode (`{S}.pt` under `latents_dir`); shifts in prompt mode.

    `cond_image=` / `target=` (the reference's `fifo_onestep` keywords reached through **kwargs) are `conditioned_image` / `targets`:
    every window then takes `ddim_step`'s segmentation branch (MoCA injection at t <= 300) with the Grounded-SAM-2 masks of
    `sam_masks` / `sam_masks_fn`, as in `fifo_ddim_sampling`.  With neither nothing is injected -- the reference itself would fail
    there (`target.endswith` on None at the first frame with t <= 300).  DAVIS inputs (`davis_data`, `davis_masks`: static masks
    indexed relative to the window, no meaning in this loop) and an image-attention UNet are refused."""
    for k in ("davis_data", "davis_masks"):
        if kwargs.pop(k, None) is not None:
            raise NotImplementedError(f"fifo_ddim_sampling_multiprompts has no DAVIS-video mode: {k} is not supported")
    refuse_multistep(ddim_sampler)
    refuse_long_window(args)
    refuse_image_attention(model)
    refuse_concat(model, conditioning)
    if save_frames and (not decode or output_dir is None):
        raise ValueError("save_frames writes decoded frames: it needs decode=True and an output_dir")
    conditioned_image = kwargs.pop("cond_image", conditioned_image)
    targets = kwargs.pop("target", targets)
    seg = multiprompt_segments(args, multiprompts, n_iterations)
    n_prompts = len(multiprompts) - 1
    text_encoder = getattr(model, "cond_stage_model", None) is not None
    if embeds is None:
        if not text_encoder:
            raise ValueError("the model has no text encoder: pass the prompt contexts as embeds=[embed_text(p) for p in prompts]")
        embeds = [model.get_learned_conditioning(p) for p in multiprompts[:-1]]
    if len(embeds) != n_prompts:
        raise ValueError(f"embeds holds {len(embeds)} contexts for {n_prompts} prompts")
    if cfg_scale != 1.0 and uc_emb is None:
        if not text_encoder:
            raise ValueError('the unconditional context is the empty prompt (funcs.py:398-399): pass uc_emb=embed_text("")')
        b = noise_shape[0]
        uc_emb = model.get_learned_conditioning(model.empty_prompt_tokens.expand(b, -1) if hasattr(model, "empty_prompt_tokens")
                                                else b * [""])
    cond = dict(conditioning or {})          # (the reference rewrites the caller's dict each iteration; this one stays as it was)
    cond["c_crossattn"] = [embeds[seg[0] if seg else 0]]
    if latents is None:
        latents = prepare_latents(args, latents_dir, ddim_sampler)

    def switch(i):                           # set_context only where j changes
        return embeds[seg[i]] if i > 0 and seg[i] != seg[i - 1] else None
    frames = fifo_ddim_sampling(args, model, cond, noise_shape, ddim_sampler, cfg_scale, uc_emb=uc_emb, latents=latents,
                                conditioned_image=conditioned_image, emit=emit, n_iterations=len(seg), batch_windows=batch_windows,
                                noises=noises, shift_noises=shift_noises, decode=decode, decode_batch=decode_batch,
                                sam_masks=sam_masks, sam_masks_fn=sam_masks_fn, targets=targets, use_graph=use_graph, seed=seed,
                                sam_capacity=sam_capacity, context_at=switch, **kwargs)
    if save_frames:
        import os
        from .io import save_frames as write_frames
        write_frames([tensor2image(fr) for fr in frames], os.path.join(output_dir, "fifo"))
    return frames


def decode_frames(model, latent_frames):
    """`model.decode_first_stage_2DAE` (ddpm3d.py:556-562) over a list of emitted latent frames [B,4,1,h,w]:
    one recorded decoder launch for all of them; returns the list of [B,3,1,8h,8w] tensors."""
    z = torch.cat(latent_frames, dim=2)
    img = model.decode_first_stage_2DAE(z)
    return [img[:, :, [i]] for i in range(img.shape[2])]


def tensor2image(batch_tensors):
    """funcs.py:630-640: [1,3,1,H,W] in [-1,1] -> uint8 [H,W,3] (a PIL image when Pillow is importable)"""
    img = torch.squeeze(batch_tensors).detach().cpu()
    img = torch.clamp(img.float(), -1., 1.)
    img = (img + 1.0) / 2.0
    arr = (img * 255).to(torch.uint8).permute(1, 2, 0).numpy()
    try:
        from PIL import Image
        return Image.fromarray(arr)
    except ImportError:
        return arr
