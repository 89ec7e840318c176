"""DDIM / DPM-Solver inpainting: the named operands of tests/golden/ddim_inpaint*.npz (tools/make_golden_ddim_inpaint.py regenerates
them by name, the tests do too) and the fp32 torch restatement of the blend and of the masked DDIM loop, op by op in the order of
`LatentDiffusion.q_sample` (ddpm3d.py:412-420), of `img_orig * mask + (1. - mask) * img` and of the tail of `p_sample_ddim`
(ddim.py:328-357), so that the blend-only mode of `moca_ddpm_step_f32` (mul / add / sub, no contraction) and the loop can be compared with them EXACTLY."""
import numpy as np
import torch

from helpers import inp

SHAPE = (1, 4, 8, 16, 16)                  # loop_base's latents
S, SCALE, T_START = 10, 12.0, 6            # loop_base's schedule rows and guidance; `decode`'s start row
# case -> (mask, eta, use_scale, rows stepped).  (a) one-channel spatial mask, left half kept; (b) frames 0-2 kept: [1,4,8,1,1]
# broadcasts over (H, W) and has the latents' channels, which the kernel reads as a "full" mask; (c) `decode` from row 6 with mask (a); (d) mask (a), eta 0, no scale
CASES = {"a": ("left", 1.0, True, S), "b": ("frames", 1.0, True, S), "c": ("left", 1.0, True, T_START), "d": ("left", 0.0, False, S)}


def mask_of(name):
    if name == "left":
        m = torch.zeros(1, 1, 1, 16, 16)
        m[..., :8] = 1.0
        return m
    m = torch.zeros(1, 4, 8, 1, 1)
    m[:, :, :3] = 1.0
    return m


def operands(case):
    """the named inputs of `case`: x_T (what `sample` starts from), x0 (the kept clip), the encode draw of case (c) and the two draws
    of every step"""
    n = CASES[case][3]
    return dict(x_T=inp("inpaint.x_T", SHAPE), x0=inp("inpaint.x0", SHAPE), enc_noise=inp("inpaint.enc_noise", SHAPE),
                noises=[inp(f"inpaint.noise{i}", SHAPE) for i in range(n)], mask_noises=[inp(f"inpaint.mnoise{i}", SHAPE) for i in range(n)])


def conds():
    fps = torch.tensor([10])
    return ({"c_crossattn": [inp("loop.ctx1", (1, 77, 128))], "fps": fps}, {"c_crossattn": [inp("loop.uctx", (1, 77, 128))], "fps": fps})


def f32(v):
    return torch.tensor(float(v), dtype=torch.float32)


def torch_blend(x, x0, mask, noise_q, sac, s1mac, scale, use_scale):
    """the blend in front of a step: q_sample (ddpm3d.py:415-420), then `img_orig * mask + (1. - mask) * img`; coefficients fp32 scalars"""
    s = f32(sac) * x0
    if use_scale:
        s = s * f32(scale)
    orig = s + f32(s1mac) * noise_q
    return orig * mask + (1. - mask) * x


def torch_ddim_tail(x, e_t, noise, coef, use_scale):
    """the tail of p_sample_ddim (ddim.py:339-357) over a row of `BaseEngine._schedule_tables`: {sqrt(a_t), sqrt(a_prev), sigma_t,
    sqrt(1 - a_t), sqrt(1 - a_prev - sigma_t^2), scale_t, scale_prev}"""
    sqrt_at, sqrt_aprev, sigma, s1m, dirc, sc, scp = (f32(v) for v in coef[:7])
    p0 = (x - s1m * e_t) / sqrt_at
    dir_xt = dirc * e_t
    nz = sigma * noise
    if use_scale:
        p0 = p0 / sc
        return sqrt_aprev * scp * p0 + dir_xt + nz
    return sqrt_aprev * p0 + dir_xt + nz


def torch_loop(x, x0, mask, eps, noises, mask_noises, coef, qcoef, use_scale):
    """upstream's masked DDIM loop over `len(eps)` table rows, walked from the last down, with the model's guided outputs `eps[i]`
    given: blend at row r, then the step of row r.  `coef` [rows][8] (`BaseEngine._schedule_tables`), `qcoef` [rows][3] (`q_rows`)"""
    n = len(eps)
    for i in range(n):
        r = n - 1 - i
        x = torch_blend(x, x0, mask, mask_noises[i], qcoef[r, 0], qcoef[r, 1], qcoef[r, 2], use_scale)
        x = torch_ddim_tail(x, eps[i], noises[i], coef[r], use_scale)
    return x


def q_rows(model, timesteps):
    """`extract_into_tensor` of the model's buffers at `timesteps`, as `q_sample` reads them -> [n][3] fp32 (scale 1 without use_scale)"""
    t = torch.as_tensor(np.asarray(timesteps), dtype=torch.int64)
    sc = model.scale_arr.detach().cpu()[t] if model.use_scale else torch.ones(t.shape[0])
    return torch.stack([model.sqrt_alphas_cumprod.detach().cpu()[t], model.sqrt_one_minus_alphas_cumprod.detach().cpu()[t], sc], 1)
