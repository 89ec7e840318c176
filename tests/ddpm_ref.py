"""Shared by tests/test_ddpm_*.py and tools/make_golden_ddpm.py: the fixture's settings, and the torch fp32 expression of one DDPM step
over the kernel's host tables -- `p_sample` over `p_mean_variance` with the loop's mask blend (ddpm3d.py:565-610,646-648), written
op by op in the reference's order so that `moca_ddpm_step_f32` (mul / add / sub, no contraction) can be compared with it EXACTLY."""
import torch

# the stand-in of the goldens: alphas_cumprod runs 0.95 .. 0.053 over eight steps
FIX = dict(timesteps=8, linear_start=0.05, linear_end=0.6, use_scale=True, mid_step=4)
LOOP_SHAPE = (1, 4, 8, 16, 16)
METHOD_SHAPE = (2, 4, 8, 16, 16)
METHOD_T = [7, 0]
GUIDE_SCALE = 7.5
TABLE_NAMES = ("sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "log_one_minus_alphas_cumprod", "posterior_variance",
               "posterior_log_variance_clipped", "posterior_mean_coef1", "posterior_mean_coef2")


def half_mask():
    """[1,1,8,16,16]: keep x0 in the left half of every frame, regenerate the right half"""
    m = torch.zeros(1, 1, *LOOP_SHAPE[2:])
    m[..., :8] = 1.0
    return m


def torch_ddpm_step(coef, t, x, eps_c, noise, eps_u=None, scale=1.0, x0_param=False, clip=False, use_scale=False, temperature=1.0,
                    mask=None, x0=None, noise_q=None):
    """-> (out, x_recon, mean).  coef [n_tab][8] = {srac, srm1, c1, c2, std, sac, s1mac, scale}, t [B] int64 (all in range)"""
    v = (x.shape[0],) + (1,) * (x.dim() - 1)
    k = [coef[t, j].view(v) for j in range(8)]
    srac, srm1, c1, c2, std, sac, s1mac, sc = k
    eps = eps_c if eps_u is None else eps_u + scale * (eps_c - eps_u)               # ddim.py:304
    x_recon = eps if x0_param else srac * x - srm1 * eps                            # :212-216, :573-576
    if clip:
        x_recon = x_recon.clamp(-1., 1.)                                            # :581
    mean = c1 * x_recon + c2 * x                                                    # :219-222
    nz = noise * temperature                                                        # :601
    nonzero = (1 - (t == 0).float()).view(v)                                        # :605
    out = mean + nonzero * std * nz                                                 # :608 with std = (0.5 * log_variance).exp() from the table
    if mask is not None:
        orig = torch_q_sample(coef, t, x0, noise_q, use_scale)
        out = orig * mask + (1. - mask) * out                                       # :648
    return out, x_recon, mean


def torch_q_sample(coef, t, x0, noise, use_scale):
    """ddpm3d.py:412-420"""
    v = (x0.shape[0],) + (1,) * (x0.dim() - 1)
    sac, s1mac, sc = (coef[t, j].view(v) for j in (5, 6, 7))
    if use_scale:
        return sac * x0 * sc + s1mac * noise
    return sac * x0 + s1mac * noise
