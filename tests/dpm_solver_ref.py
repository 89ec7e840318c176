"""References of tests/test_dpm_solver_cpu.py and tests/test_dpm_solver_gpu.py: DPM-Solver++(2M) (Lu et al., 2022; data prediction,
multistep, midpoint form) on the DDIM sampler's schedule rows, restated from the formulas alone -- nothing here imports the
package's table builder, engine or sampler class.

Row i of an eta-0 schedule takes the latents from level (a, s) = (ddim_alphas[i], ddim_scale_arr[i]) to (ddim_alphas_prev[i],
ddim_scale_arr_prev[i]) (s = 1 without `use_scale`), the model evaluated at ddim_timesteps[i].  With alpha = sqrt(a) s,
sigma = sqrt(1 - a), lam = log(alpha / sigma) and h = lam_prev - lam:

    p0 = (x - sqrt(1 - a) eps) / sqrt(a) [/ s]          c_x = sigma_prev / sigma          c_0 = -alpha_prev expm1(-h)
    x' = c_x x + c_0 p0 + c_1 (p0 - p0_prev)            c_1 = 0.5 c_0 h / h_prev, or 0: a first-order step

A trajectory over the first n rows walks i = n - 1 .. 0; rows with h == 0 are identities and the ones at the clean end are not stepped;
c_1 = 0 on the first stepped row, at order 1, and with `lower_order_final` on the last stepped row.

Three forms: `tables64` / `step64` in float64; `step32`, the fp32 torch evaluation in the kernel's order of operations (no FMA: the
expected output of `moca_base_ddim_step_f32` with MOCA_BASE_MULTISTEP, bit for bit); and the Gaussian model whose probability-flow
ODE has a closed form."""
import numpy as np
import torch

F32, F64 = torch.float32, torch.float64
MULTISTEP, SCALE_BIT = 2, 1                              # include/moca_hip.h: MOCA_BASE_MULTISTEP, MOCA_BASE_SCALE


def schedule64(sampler, n_rows=None):
    """(a, a_prev, s, s_prev) of the sampler's first n_rows schedule rows as float64 arrays"""
    n = len(sampler.ddim_timesteps) if n_rows is None else n_rows
    f = lambda v: np.asarray(v, dtype=np.float64)[:n].copy()
    a, ap = f(sampler.ddim_alphas), f(sampler.ddim_alphas_prev)
    if sampler.use_scale:
        return a, ap, f(sampler.ddim_scale_arr), f(sampler.ddim_scale_arr_prev)
    return a, ap, np.ones(n), np.ones(n)


def level(a, s):
    """(alpha, sigma, lam) of a level"""
    alpha, sigma = np.sqrt(a) * s, np.sqrt(1. - a)
    return alpha, sigma, np.log(alpha / sigma)


def tables64(a, ap, s, sp, order=2, lower_order_final=True):
    """-> dict of float64 arrays over the rows: sqrt_a, c0, c1, sqrt_1ma, cx, scale, h, and `stepped`: the row indices a trajectory
    steps, in its order (descending)"""
    n = len(a)
    out = {k: np.zeros(n) for k in ("c0", "c1", "h")}
    out.update(sqrt_a=np.sqrt(a), sqrt_1ma=np.sqrt(1. - a), scale=s.copy(), cx=np.ones(n))
    for i in range(n):
        alpha, sigma, lam = level(a[i], s[i])
        alpha_p, sigma_p, lam_p = level(ap[i], sp[i])
        out["h"][i] = lam_p - lam
        if out["h"][i] != 0:
            out["cx"][i] = sigma_p / sigma
            out["c0"][i] = -alpha_p * np.expm1(-out["h"][i])
    moving = [i for i in range(n) if out["h"][i] != 0]
    clean_end = min(moving) if moving else n
    stepped = list(range(n - 1, clean_end - 1, -1))
    prev = None                                          # the previous step that moved: an identity row never is one
    for k, i in enumerate(stepped):
        if out["h"][i] == 0:
            continue
        last = i == clean_end
        if order == 2 and prev is not None and not (lower_order_final and last):
            out["c1"][i] = 0.5 * out["c0"][i] * out["h"][i] / out["h"][prev]
        prev = i
    out["stepped"] = stepped
    return out


def coef_table(tab):
    """the [n][8] float64 table in the kernel's column order: {sqrt(a_t), c_0, c_1, sqrt(1 - a_t), c_x, scale_t, 0, 0}"""
    n = len(tab["c0"])
    c = np.zeros((n, 8))
    for col, k in enumerate(("sqrt_a", "c0", "c1", "sqrt_1ma", "cx", "scale")):
        c[:, col] = tab[k]
    return c


def step64(x, eps, p0_prev, row, use_scale):
    """one step in float64 on a coefficient row (8 values); p0_prev None or c_1 == 0: first order -> (x', p0)"""
    r = [float(v) for v in row]
    x, eps = x.to(F64), eps.to(F64)
    p0 = (x - r[3] * eps) / r[0]
    if use_scale:
        p0 = p0 / r[5]
    xn = r[4] * x + r[1] * p0
    if r[2] != 0:
        xn = xn + r[2] * (p0 - p0_prev.to(F64))
    return xn, p0


def ddim_tail64(x, eps, a, ap, s, sp, use_scale):
    """the tail of p_sample_ddim (ddim.py:339-356) at sigma_t = 0 in float64 -> (x_prev, pred_x0)"""
    x, eps = x.to(F64), eps.to(F64)
    a, ap, s, sp = float(a), float(ap), float(s), float(sp)         # (python floats: a numpy scalar on the left would take the product over)
    p0 = (x - float(np.sqrt(1. - a)) * eps) / float(np.sqrt(a))
    d = float(np.sqrt(1. - ap)) * eps
    if use_scale:
        p0 = p0 / s
        return float(np.sqrt(ap)) * sp * p0 + d, p0
    return float(np.sqrt(ap)) * p0 + d, p0


def step32(x, e_c, e_u, hist, row, cfg_scale, use_scale):
    """the kernel's step in fp32 torch ops, in its order, on an fp32 coefficient row [8]: guidance e_u + s (e_c - e_u) (e_u None: none),
    p0 as DDIM's, x' = (c_x x + c_0 p0) + c_1 (p0 - hist) with the history looked at only where c_1 != 0 -> (x', p0 = the new history)"""
    row = row.to(F32)
    x, e = x.to(F32), e_c.to(F32)
    if e_u is not None:
        e = e_u.to(F32) + torch.tensor(cfg_scale, dtype=F32) * (e - e_u.to(F32))
    p0 = (x - row[3] * e) / row[0]
    if use_scale:
        p0 = p0 / row[5]
    xn = row[4] * x + row[1] * p0
    if float(row[2]) != 0:
        xn = xn + row[2] * (p0 - hist.to(F32))
    return xn, p0


def ddim_tail32(x, e, row7, use_scale):
    """the fp32 DDIM tail at sigma 0 on `BaseEngine`'s row {sqrt(a_t), sqrt(a_prev), 0, sqrt(1 - a_t), sqrt(1 - a_prev), scale_t,
    scale_prev}, in `ddim_tail`'s order of operations"""
    r = row7.to(F32)
    x, e = x.to(F32), e.to(F32)
    p0 = (x - r[3] * e) / r[0]
    d = r[4] * e
    if use_scale:
        p0 = p0 / r[5]
        return r[1] * r[6] * p0 + d, p0
    return r[1] * p0 + d, p0


# ---- a model with a closed form: data ~ N(0, s^2), x_a = sqrt(a) x_0 + sqrt(1 - a) n has variance a s^2 + 1 - a ---------------------
def gaussian_eps(x, a, s):
    """the exact noise prediction E[n | x_a = x] = sqrt(1 - a) x / (a s^2 + 1 - a)"""
    a = float(a)
    return float(np.sqrt(1. - a)) * x / (a * s * s + 1. - a)


def gaussian_exact(x_T, a_T, a_end, s):
    """the probability-flow ODE's solution at level a_end from x_T at level a_T: the standard deviations' ratio"""
    a_T, a_end = float(a_T), float(a_end)
    return x_T * float(np.sqrt(a_end * s * s + 1. - a_end) / np.sqrt(a_T * s * s + 1. - a_T))


def gaussian_run(tab, a, x_T, s, dtype=F64):
    """the stepped rows of `tab` on the Gaussian model: float64 throughout, or with the table rounded to fp32 and `step32`"""
    c = coef_table(tab)
    x, hist = x_T.to(dtype), None
    for i in tab["stepped"]:
        eps = gaussian_eps(x.to(F64), a[i], s)
        if dtype == F64:
            x, hist = step64(x, eps, hist, c[i], False)
        else:
            x, hist = step32(x, eps.to(F32), None, hist, torch.from_numpy(c[i].astype(np.float32)), 1.0, False)
    return x


def rel_err(x, exact):
    return float(((x.to(F64) - exact.to(F64)).abs() / exact.to(F64).abs()).max())
