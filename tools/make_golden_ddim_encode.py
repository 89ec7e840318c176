#!/usr/bin/env python3
"""Generate the goldens of `DDIMSampler.encode`, the deterministic DDIM inversion, on the CPU.  The reference's sampler has no `encode`
of its own; what it has is the arithmetic: one inversion step is the tail of the REAL `p_sample_ddim` (lvdm/models/samplers/ddim.py:
328-357) on a copy of the sampler whose six tables are swapped --

    ddim_alphas <-> ddim_alphas_prev, ddim_scale_arr <-> ddim_scale_arr_prev, ddim_sigmas = 0,
    ddim_sqrt_one_minus_alphas = np.sqrt(1. - ddim_alphas_prev)        (built as ddim.py:102 builds it)

-- called for i = 0 .. t_enc - 1 ascending with index = i and t = ddim_timesteps[i].  Every latent below comes out of that real method.

  ddim_encode.npz        the real reduced-width UNet inside the real `DiffusionWrapper` through the real `LatentDiffusion.apply_model`,
                         loop_base's contexts and fps, x0 = inp("v2v.x0", [1,4,8,16,16]), S = 10, t_enc = 6, eta 0, use_scale, for
                         guidance 1.0 and 3.0 (keys g1_* / g3_*): x_T, the six intermediates, and the round-trip clip
                         rt = decode(x_T, c, 6, g, uc) of the real `decode`.  queue: the deterministic `ddim_inversion` queue of
                         z = inp("ddim_encode.z", [1,4,4,16,16]), N = 10, guidance 1: frame i = X_i[:, :, idx(i)].
                         Fixture conditions, the reference against itself, ASSERTED here for both guidances:
                           * evaluating the model at the next level's timestep (t = ddim_timesteps[i + 1]),
                           * shifting the level index by one (index = i + 1),
                           * stopping one step early (t_enc = 5)
                           each move x_T by more than 3 x TOL_BASE of max|x_T|;
                           * the inversion round trip lands closer to x0 than half of the round trip through `stochastic_encode`
                             (index 6, inp("v2v.enc_noise"), as `v2v_ddim_sampling` encodes) -- distances as max|. - x0| / max|x0|.
  ddim_encode_cases.npz  the coefficient rows of every inversion step (S = 10 and 50 with use_scale, S = 10 without), evaluated here
                         from the reference sampler's own tables as fp32 numpy scalars; the (timestep, level index) sequence of
                         t_enc in {1, 6, 10} logged from the real `p_sample_ddim` / `apply_model` calls; one scripted-eps step
                         (`FakeModel`) with guidance 3 and one without.

    python tools/make_golden_ddim_encode.py

Same recipe as tools/make_golden_v2v.py (whose helpers it imports): inputs are regenerated bit-identically by name, the fp32 square
roots of schedule scalars are pinned to the correctly rounded result -- here `Tensor.sqrt` too, which `p_sample_ddim` calls -- so the
goldens do not depend on the CPU the tool ran on."""
import contextlib
import copy
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as MG  # noqa: E402
import make_golden_v2v as V  # noqa: E402
from make_golden_v2v import FACTOR, TOL_BASE, quiet, relerr  # noqa: E402

SHAPE = (1, 4, 8, 16, 16)
ZSHAPE = (1, 4, 4, 16, 16)
S, T_ENC, N_QUEUE = 10, 6, 10
SCALES = (1.0, 3.0)


@contextlib.contextmanager
def pinned_roots():
    """`pinned_sqrt` of the v2v tool, extended to the method form `t.sqrt()` that p_sample_ddim uses (ddim.py:339,343,355)"""
    real = torch.Tensor.sqrt
    with V.pinned_sqrt() as changed:
        torch.Tensor.sqrt = lambda self: torch.sqrt(self)
        try:
            yield changed
        finally:
            torch.Tensor.sqrt = real


def swapped(s):
    """a copy of the sampler `s` with the six tables of one inversion step in the places p_sample_ddim reads (see the module docstring)"""
    r = copy.copy(s)
    r.ddim_alphas, r.ddim_alphas_prev = s.ddim_alphas_prev, s.ddim_alphas
    if s.use_scale:
        r.ddim_scale_arr, r.ddim_scale_arr_prev = s.ddim_scale_arr_prev, s.ddim_scale_arr
    r.ddim_sigmas = np.zeros(len(s.ddim_timesteps))
    r.ddim_sqrt_one_minus_alphas = np.sqrt(1. - s.ddim_alphas_prev)
    return r


def ref_encode(D, s, x0, cond, t_enc, scale=1.0, uc=None, t_shift=0, index_shift=0):
    """t_enc inversion steps by the real p_sample_ddim on the swapped copy of `s` -> (x_T, [state after every step])"""
    sw = swapped(s)
    real = D.noise_like
    D.noise_like = lambda shp, dev, repeat=False: torch.zeros(shp)       # (sigma is 0: nothing of the draw reaches the result)
    x, inter = x0, []
    try:
        with torch.no_grad(), pinned_roots():
            for i in range(t_enc):
                t = torch.full((x0.shape[0],), int(s.ddim_timesteps[i + t_shift]), dtype=torch.long)
                x, _ = sw.p_sample_ddim(x, cond, t, index=i + index_shift, unconditional_guidance_scale=scale, unconditional_conditioning=uc)
                inter.append(x)
    finally:
        D.noise_like = real
    return x, inter


def coef_rows(s):
    """[S][7] = sqrt(a_cur), sqrt(a_next), 0, sqrt(1 - a_cur), sqrt(1 - a_next), s_cur, s_next per inversion step, from the reference
    sampler's tables: fp32 scalars, numpy's (correctly rounded) roots; sqrt(1 - a_cur) from np.sqrt(1. - ddim_alphas_prev) as a table"""
    f32 = np.float32
    n = len(s.ddim_timesteps)
    s1m = np.sqrt(1. - s.ddim_alphas_prev)
    rows = np.zeros((n, 7), np.float32)
    for i in range(n):
        a_cur, a_next = f32(s.ddim_alphas_prev[i]), f32(s.ddim_alphas[i])
        sc = (f32(s.ddim_scale_arr_prev[i]), f32(s.ddim_scale_arr[i])) if s.use_scale else (f32(1), f32(1))
        rows[i] = (np.sqrt(a_cur), np.sqrt(a_next), f32(0), f32(s1m[i]), np.sqrt(f32(1.) - a_next)) + sc
    return rows


def sample_case(D, ddpm3d):
    wrapper = ddpm3d.DiffusionWrapper({"target": "lvdm.modules.networks.openaimodel3d.UNetModel", "params": dict(MG.REDUCED)},
                                      "crossattn").eval()
    MG.fill(wrapper.diffusion_model, 11)

    class Model(MG.FakeModel):
        model = wrapper
        apply_model = ddpm3d.LatentDiffusion.apply_model

    model = Model()
    fps = torch.tensor([10])
    cond = {"c_crossattn": [MG.inp("loop.ctx1", (1, 77, 128))], "fps": fps}
    uc = {"c_crossattn": [MG.inp("loop.uctx", (1, 77, 128))], "fps": fps}
    x0 = MG.inp("v2v.x0", SHAPE)
    n_enc = MG.inp("v2v.enc_noise", SHAPE)
    s = D.DDIMSampler(model)
    s.make_schedule(S, ddim_eta=0.0, verbose=False)
    need = FACTOR * TOL_BASE
    dist = lambda x: relerr(x, x0)
    out = {}
    with torch.no_grad(), V.pinned_sqrt():
        x_sto = s.stochastic_encode(x0, torch.tensor([T_ENC]), noise=n_enc)
    for g in SCALES:
        tag = f"g{g:g}"
        t0 = time.time()
        x_T, inter = ref_encode(D, s, x0, cond, T_ENC, g, uc)
        moved = {"next level's timestep": relerr(ref_encode(D, s, x0, cond, T_ENC, g, uc, t_shift=1)[0], x_T),
                 "level index + 1": relerr(ref_encode(D, s, x0, cond, T_ENC, g, uc, index_shift=1)[0], x_T),
                 "one step early": relerr(inter[T_ENC - 2], x_T)}
        for k, v in moved.items():
            print(f"[encode] guidance {g}: sensitivity, {k}: x_T moves by {v:.3e} of max|x_T| (need > {need:.2e}, margin {v / need:.1f} x)")
        assert all(v > need for v in moved.values()), "the fixture does not separate a wrong inversion step from TOL_BASE: change the fixture"
        with torch.no_grad(), quiet(), pinned_roots():
            rt = s.decode(x_T, cond, T_ENC, g, uc)
            rt_sto = s.decode(x_sto, cond, T_ENC, g, uc)
        d_inv, d_sto = dist(rt), dist(rt_sto)
        print(f"[encode] guidance {g}: round trip to x0: inversion {d_inv:.3f}, stochastic_encode {d_sto:.3f} of max|x0| "
              f"({time.time() - t0:.1f}s; x_T std {x_T.std():.3f})")
        assert d_inv < 0.5 * d_sto, "the inversion round trip is not closer to x0 than half of the stochastic round trip"
        out.update({f"{tag}_x_T": x_T, f"{tag}_inter": torch.stack(inter), f"{tag}_rt": rt,
                    f"{tag}_sens": np.asarray(list(moved.values())), f"{tag}_dist": np.asarray([d_inv, d_sto])})
    # ---- the deterministic queue of ddim_inversion: frame i = X_i[:, :, idx(i)]
    z = MG.inp("ddim_encode.z", ZSHAPE)
    _, states = ref_encode(D, s, z, cond, N_QUEUE)
    idx = [max(0, i - (N_QUEUE - ZSHAPE[2])) for i in range(N_QUEUE)]                # ddim.py:1014
    out["queue"] = torch.stack([x[:, :, j] for x, j in zip(states, idx)], dim=2)
    out["queue_idx"] = np.asarray(idx)
    MG.save("ddim_encode", S=np.asarray(S), t_enc=np.asarray(T_ENC), scales=np.asarray(SCALES), **out)


def index_and_step_cases(D):
    out = {}
    for tag, n, use_scale in (("S10", 10, True), ("S50", 50, True), ("S10_noscale", 10, False)):
        fm = MG.FakeModel()
        fm.use_scale = use_scale
        s = D.DDIMSampler(fm)
        s.make_schedule(n, ddim_eta=1.0, verbose=False)          # (eta plays no part: the swapped sigmas are 0)
        out[f"coef_{tag}"] = coef_rows(s)
    # ---- (timestep, level index) of every step, logged where the real method and the model see them
    log, idx_log = [], []

    class Logger(MG.FakeModel):
        def apply_model(self, x, t, c, **kw):
            log.append(int(t[0]))
            return torch.zeros_like(x)

    s = D.DDIMSampler(Logger())
    s.make_schedule(S, ddim_eta=0.0, verbose=False)
    orig = D.DDIMSampler.p_sample_ddim

    def spy(self, x, c, t, index, **kw):
        idx_log.append(int(index))
        return orig(self, x, c, t, index=index, **kw)
    D.DDIMSampler.p_sample_ddim = spy
    try:
        for t_enc in (1, 6, 10):
            log.clear(); idx_log.clear()
            ref_encode(D, s, torch.zeros(1, 4, 2, 2, 2), None, t_enc)
            assert len(log) == len(idx_log) == t_enc
            out[f"encode_S{S}_t{t_enc}"] = np.asarray([log, idx_log], dtype=np.int64)       # [2][t_enc]: timesteps, level indices
            print(f"[encode] t_enc={t_enc}: timesteps {log} levels {idx_log}")
    finally:
        D.DDIMSampler.p_sample_ddim = orig
    # ---- one scripted-eps step, with and without guidance
    fm = MG.FakeModel()
    s = D.DDIMSampler(fm)
    s.make_schedule(S, ddim_eta=0.0, verbose=False)
    shape = (1, 4, 3, 5, 7)
    for tag, index, g in (("guided", 3, 3.0), ("plain", 0, 1.0)):
        x, e_c, e_u = (MG.inp(f"ddim_encode.step.{tag}.{k}", shape) for k in ("x", "ec", "eu"))
        fm.queue = [e_c.clone(), e_u.clone()]
        sw = swapped(s)
        real = D.noise_like
        D.noise_like = lambda shp, dev, repeat=False: torch.zeros(shp)
        try:
            with torch.no_grad(), pinned_roots():
                t = torch.full((1,), int(s.ddim_timesteps[index]), dtype=torch.long)
                xn, p0 = sw.p_sample_ddim(x, {"c_crossattn": [None]}, t, index, unconditional_guidance_scale=g,
                                          unconditional_conditioning={"c_crossattn": [None]})
        finally:
            D.noise_like = real
        assert len(fm.queue) == (0 if g != 1.0 else 1)
        out[f"step_{tag}_x_next"], out[f"step_{tag}_pred_x0"] = xn, p0
        out[f"step_{tag}_index"], out[f"step_{tag}_scale"] = np.asarray(index), np.asarray(g)
    MG.save("ddim_encode_cases", **out)


def main():
    torch.set_num_threads(8)
    MG.import_reference()
    from lvdm.models import ddpm3d
    D = V.patched_sampler_module()
    index_and_step_cases(D)
    sample_case(D, ddpm3d)


if __name__ == "__main__":
    main()
