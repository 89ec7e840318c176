"""What the samplers (`sampler`, `ddpm`, `fifo`, `fifo_graph`) all ask of a model and its conditioning, once: where the UNet and its
conditioning key are, `apply_model`'s normalisation of `cond`, the concatenated context, the fps rows, the refusals of the FIFO loop,
the conditioning-image rows, the schedule-index check, and the ONE place that decides how the two classifier-free-guidance branches
reach the UNet (`guidance_eps`).  A leaf: of the package it imports `unet` alone (`lib` and `ops` would be fine, a sampler module
never), so the four modules above import each other in one direction (conditioning <- fifo_graph <- sampler, ddpm <- fifo)."""
from __future__ import annotations

import torch

from .unet import same_fps  # noqa: F401  (re-exported)

# conditioning latents concatenated to x along the channel axis + a cross-attention context (ddpm3d.py:713-717,724-733,747-759)
HYBRID_KEYS = ("hybrid", "hybrid-adm", "hybrid-time", "hybrid-adm-mask", "hybrid-time-adm")
# keys whose branch calls the UNet with context=None: the reference's own UNet fails there (openaimodel3d.py:547,
# `context.repeat_interleave` on None)
CONTEXT_FREE_KEYS = (None, "concat", "adm", "resblockcond", "concat-time-mask", "concat-adm-mask")


def _f32c(t):
    return t.contiguous() if t.dtype == torch.float32 else t.float().contiguous()


def unet_of(model):
    """`model.model.diffusion_model`, None for a model without one"""
    return getattr(getattr(model, "model", None), "diffusion_model", None)


def conditioning_key(model):
    return getattr(getattr(model, "model", None), "conditioning_key", None)


def as_cond_dict(cond, key="crossattn"):
    """apply_model's normalisation of `cond` (ddpm3d.py:513-520): a tensor or a list is `c_crossattn` (`c_concat` under 'concat')"""
    if isinstance(cond, dict):
        return cond
    if not isinstance(cond, list):
        cond = [cond]
    return {'c_concat' if key == 'concat' else 'c_crossattn': cond}


def context(cond):
    """the cross-attention context of a cond dict as DiffusionWrapper.forward builds it (ddpm3d.py:711)"""
    return torch.cat(cond["c_crossattn"], 1)


def one_fps(fp):
    """one fps for a whole branch: of a tensor the first value"""
    return fp if isinstance(fp, int) else torch.as_tensor(fp).reshape(-1)[:1]


def fps_rows(fp, B, T=None, dev=None):
    """the fps of B videos, a tensor holding one value for all of them or one per video.  T None: one row per video as the UNet takes
    them (an int stays an int); T frames: the [B*T] int64 rows of a plan."""
    if isinstance(fp, int):
        return fp if T is None else torch.full((B * T,), fp, dtype=torch.int64, device=dev)
    fp = torch.as_tensor(fp, device=dev).reshape(-1)
    fp = fp if fp.shape[0] == B else fp[:1].expand(B)
    return fp if T is None else fp.to(torch.int64).repeat_interleave(T)


def refuse_image_attention(model):
    """The MoCA loop's two-prompt context is 154 tokens; an image-attention UNet would split it 77 / 77 into "text" and "image"
    tokens by the reference's rule (attention.py:82-84).  That mode is not supported: raise instead of computing it."""
    if getattr(unet_of(model), "use_image_attention", False):
        raise NotImplementedError("FIFO / MoCA sampling with an image-attention UNet (use_image_attention=True) is not supported: "
                                  "its 154-token two-prompt context would be read as 77 text + 77 image tokens")


def refuse_long_window(args):
    """FIFO / MoCA windows are at most 16 frames: the one-graph loop (ring queue, per-window timestep tables, batched windows) is
    built and measured for the 16-frame tile of the temporal attention; the UNet alone takes up to 32 frames (UNetModel.forward)"""
    if args.video_length > 16:
        raise ValueError(f"video_length = {args.video_length}: FIFO sampling takes windows of video_length <= 16 frames "
                         f"(base_ddim_sampling / v2v_ddim_sampling take up to 32)")


def refuse_concat(model, cond=None):
    """FIFO / MoCA sampling has no channel-concatenated conditioning: the reference's loop hands every window the whole `cond`
    and never slices `c_concat` along the queue, so there is no behaviour to reproduce.  Raise instead of computing something."""
    key = conditioning_key(model)
    if key in HYBRID_KEYS or (isinstance(cond, dict) and cond.get("c_concat") is not None):
        raise NotImplementedError(f"FIFO / MoCA sampling with channel-concatenated conditioning (conditioning_key={key!r}, c_concat) is "
                                  "not supported: the queue's windows would each need their own slice of c_concat; use "
                                  "base_ddim_sampling")


def cond_image_rows(cond_image, Cc, HW, device):
    """the conditioning image(s) of ddim_step as fp32 rows [n, Cc, HW] (ddim.py:573-578): zeros without one, a 3-channel image gets a
    fourth channel of ones"""
    if cond_image is None:
        return torch.zeros(1, Cc, HW, dtype=torch.float32, device=device)
    ci = cond_image.to(device)
    if ci.shape[1] != Cc:
        if ci.shape[1] != 3:
            raise ValueError(f"Conditional image must have 3 or 4 channels, got {ci.shape[1]}")
        ci = torch.cat([ci, torch.ones_like(ci[:, :1])], dim=1)
    return _f32c(ci).reshape(-1, Cc, HW)


def check_schedule_index(t, B, n, what="schedule index"):
    """`t` as a tensor holding one index into an n-entry schedule table per sample, on either device: a host tensor is range-checked
    here (IndexError, as `gather`), a device tensor is gathered by the kernel without a host read (out of range: that sample is NaN)"""
    t = torch.as_tensor(t)
    if t.dim() != 1 or t.shape[0] != B:
        raise ValueError(f"t must hold one {what} per sample, shape [{B}], got {tuple(t.shape)}")
    if not t.is_cuda and t.numel() and (int(t.min()) < 0 or int(t.max()) >= n):
        raise IndexError(f"{what} {t.tolist()} is out of bounds for the {n}-entry schedule table")
    return t


def guidance_eps(model, x, t, c, uc, scale, *, share_prefix=True, cfg_mode="batched", rows=None, share_any=False, batch=True, **kwargs):
    """The UNet evaluation(s) of one classifier-free-guidance step (ddim.py:290-304,362-374) -> (e_c, e_u), or the single eps without
    guidance (`uc` None or scale 1).  The routes, in the order they are tried:
      concurrent  `forward_concurrent`: the branches as two B-sized graphs on two streams (`cfg_mode == "concurrent"`);
      shared      `forward_segments(shared_x=True)`: ONE forward that computes everything before the first cross-attention once
                  (same x, same t; it adds ONE fps embedding, so the branches' fps must be equal), `share_prefix`;
      batch       `apply_model` on [x, x] with the contexts stacked: needs contexts of one shape;
      two calls   `apply_model` per branch, with `c` and `uc` as they came.
    `pair` below (dict conditionings of `c_crossattn` / `fps` only, contexts of one shape, 2 B <= 64) is what concurrent and batch
    ask for, and shared too unless the caller says `share_any`.  Extra `kwargs` go to `apply_model`; the shared route hands on
    `features_adapter` alone (the same maps for both branches, doubled along the batch for [x, x]) and the concurrent route is not
    taken with adapter maps or with `no_concurrent=True`.

    What the three callers set, i.e. where they differ:
      DDIMSampler._cfg_eps      the sampler's `share_prefix` and `cfg_mode`, nothing else.
      DDIMSampler.unet_windows  `rows=W`: x holds W windows of ONE video, so every fps handed to the UNet becomes W rows of the branch's
                                first value.  `share_any`: the shared route also takes contexts of unequal length (154 conditional
                                tokens against 77 unconditional ones: the MoCA loop's case) and is not capped at 2 W <= 64; batch then
                                asks only for one context shape and fps of one kind (both int or both tensors).  Never concurrent.
                                Adapter maps are unknown here: `features_adapter` reaches `apply_model` as it came and the shared
                                route not at all.
      DdpmMixin._ddpm_step      `share_prefix` = "no extra kwargs and `DdpmEngine.supported`", so that the host-issued step shares
                                exactly where the one-graph step does: with `share_any` (unequal lengths; a bare tensor or a list is
                                `c_crossattn`), and `batch=False`: never [x, x], never concurrent.
    With unequal int fps (or an int against a tensor) `_cfg_eps`'s batch route gives BOTH branches the conditional fps."""
    B = x.shape[0]
    fr = (lambda f: f) if rows is None else (lambda f: fps_rows(one_fps(f), rows, dev=x.device))
    branch = (lambda d: d) if rows is None else (lambda d: dict(d, fps=fr(d["fps"])))
    if uc is None or scale == 1.:
        return model.apply_model(x, t, branch(c), **kwargs)
    unet, key = unet_of(model), conditioning_key(model)
    fa = kwargs.get("features_adapter") if rows is None else None
    cd, ud = (as_cond_dict(c, key), as_cond_dict(uc, key)) if share_any else (c, uc)
    # (the contexts are concatenated only where a route that reads them can still be taken)
    have = (share_prefix or batch) and isinstance(cd, dict) and isinstance(ud, dict) and (share_any or 2 * B <= 64)
    pair = False
    if have:
        cc, cu = context(cd), context(ud)
        f_c, f_u = cd.get("fps", 16), ud.get("fps", 16)
        pair = batch and cc.shape == cu.shape and (set(cd.keys()) == set(ud.keys()) <= {"c_crossattn", "fps"} if rows is None
                                                   else isinstance(f_c, int) == isinstance(f_u, int))
    if pair and rows is None and cfg_mode == "concurrent" and hasattr(unet, "forward_concurrent") and not kwargs.get("no_concurrent") \
            and fa is None:
        e_c, e_u = unet.forward_concurrent([dict(x=x, timesteps=t, context=cc, fps=f_c), dict(x=x, timesteps=t, context=cu, fps=f_u)])
    elif have and (pair or share_any) and share_prefix and hasattr(unet, "forward_segments") and key == "crossattn" \
            and same_fps([f_c, f_u]):
        fr_c = fr(f_c)
        e = unet.forward_segments(x, t, [cc, cu], fps=[fr_c, fr_c if f_u is f_c else fr(f_u)], shared_x=True, features_adapter=fa)
        e_c, e_u = e[:B], e[B:]
    elif pair:
        cond = {"c_crossattn": [torch.cat([cc, cu], 0)]}
        if "fps" in cd:
            per = fr if rows is not None else (lambda f: torch.as_tensor(f).reshape(-1).expand(B))
            cond["fps"] = f_c if isinstance(f_c, int) else torch.cat([per(f_c), per(f_u)], 0)
        tt = torch.as_tensor(t, device=x.device).reshape(-1)          # [B] per sample, or (FIFO, B == 1) per frame: either way twice
        if fa is not None:                                            # [x, x]: the frames of every map twice
            kwargs = dict(kwargs, features_adapter=[torch.cat([f, f], 0) for f in fa])
        e = model.apply_model(torch.cat([x, x], 0), torch.cat([tt, tt], 0), cond, **kwargs)
        e_c, e_u = e[:B], e[B:]
    else:
        e_c = model.apply_model(x, t, branch(c), **kwargs)
        e_u = model.apply_model(x, t, branch(uc), **kwargs)
    return e_c, e_u
