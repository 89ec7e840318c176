"""CPU: DDIM / DPM-Solver inpainting without a GPU -- the table rows the blend reads against the model's own buffers, the fp32 torch
restatement of upstream's masked DDIM loop against the goldens of the REAL reference (tests/golden/ddim_inpaint*.npz,
tools/make_golden_ddim_inpaint.py) EXACTLY, the engine keys, the argument contracts of `sample` / `decode` and of the C entry, and
the pixel-to-latent mask reduction of the drivers."""
import ctypes as C

import numpy as np
import pytest
import torch

from ddim_inpaint_ref import CASES, S, SCALE, SHAPE, T_START, conds, mask_of, operands, q_rows, torch_loop
from helpers import REDUCED, golden

UNET = {"target": "lvdm.modules.networks.openaimodel3d.UNetModel", "params": REDUCED}


def _model(use_scale=True):
    from moca_video_amd import DenoiseModel
    return DenoiseModel(UNET, use_scale=use_scale)


def _sampler(model, eta=1.0, cls=None):
    from moca_video_amd.sampler import DDIMSampler
    s = (cls or DDIMSampler)(model)
    s.make_schedule(S, ddim_eta=eta, verbose=False)
    return s


@pytest.mark.parametrize("use_scale", [True, False])
def test_q_table_rows_are_the_models_buffers_at_the_ddim_timesteps(use_scale):
    """the rows the blend reads -- columns {sac, s1mac, scale} of the model's DDPM table at ddim_timesteps, gathered by the kernel from
    the plan's timestep rows -- are `extract_into_tensor` of sqrt_alphas_cumprod / sqrt_one_minus_alphas_cumprod / scale_arr at those
    timesteps, bit for bit: not values recomputed from the sampler's ddim_alphas (whose fp32 roots differ in the last bit)"""
    from moca_video_amd.sampler import sqrt_f32
    m = _model(use_scale)
    s = _sampler(m)
    coef = torch.from_numpy(m._ddpm_host()["coef"])
    assert coef.dtype == torch.float32 and coef.shape == (1000, 8)
    t = torch.as_tensor(np.asarray(s.ddim_timesteps), dtype=torch.int64)
    q = coef[t][:, 5:8]
    assert torch.equal(q, q_rows(m, s.ddim_timesteps))
    assert torch.equal(q[:, 2], torch.ones(S)) != use_scale
    assert torch.equal(coef[t[:T_START]][:, 5:8], q[:T_START])                       # `decode`'s engine walks the first t_start rows
    assert not torch.equal(q[:, 0], sqrt_f32(np.asarray(s.ddim_alphas)))             # what a table "recomputed from ddim_alphas" would hold


@pytest.mark.parametrize("case", list(CASES))
def test_torch_restatement_reproduces_the_reference_golden_exactly(case):
    """upstream's loop -- blend at row r with the model's q_sample rows, then the DDIM tail of row r -- restated in fp32 torch over the
    product's own host tables and the recorded guided model outputs equals the real reference's result bit for bit"""
    from moca_video_amd.fifo_graph import BaseEngine
    mask_name, eta, use_scale, n_rows = CASES[case]
    g, eps = golden("ddim_inpaint"), torch.from_numpy(golden(f"ddim_inpaint_eps_{case}")["eps"])
    assert (int(g["S"]), float(g["scale"]), int(g["t_start"])) == (S, SCALE, T_START) and eps.shape == (n_rows,) + SHAPE
    m = _model(use_scale)
    s = _sampler(m, eta)
    coef, t_table = BaseEngine._schedule_tables(s, n_rows)
    o = operands(case)
    x_start = o["x_T"] if n_rows == S else torch.from_numpy(g[case + "__x_enc"])
    got = torch_loop(x_start, o["x0"], mask_of(mask_name), list(eps), o["noises"], o["mask_noises"], coef, q_rows(m, t_table), use_scale)
    ref = torch.from_numpy(g[case])
    print(f"[exact] case {case}: max|got - ref| = {(got - ref).abs().max().item():.3e}")
    assert torch.equal(got, ref)
    assert (g[case + "__sens"] > 3 * 1.7e-2).all()                                   # what the tool asserted: 3 x TOL_BASE


def test_engine_keys_separate_masked_from_unmasked_and_the_mask_kinds():
    from moca_video_amd.fifo_graph import BaseEngine, DpmEngine
    from moca_video_amd.sampler import DPMSolverSampler
    m = _model()
    cond, uc = conds()
    x = torch.zeros(SHAPE)
    for cls, s in ((BaseEngine, _sampler(m)), (DpmEngine, _sampler(m, 0.0, DPMSolverSampler))):
        key = lambda mask=None, n_rows=None: cls.key(s, x, cond, uc, SCALE, None, n_rows, mask)
        plain, c0, full = key(), key(mask_of("left")), key(mask_of("frames"))
        assert plain == cls.key(s, x, cond, uc, SCALE) and plain[-1] is None
        assert (c0[-1], full[-1]) == ("c0", "full") and len({plain, c0, full}) == 3
        assert key(torch.ones(16, 16)) == c0 and key(torch.ones(SHAPE)) == full        # another mask of the same kind: the same engine
        assert key(mask_of("left"), T_START) != c0


def test_sample_and_decode_refuse_inconsistent_mask_arguments():
    from moca_video_amd.sampler import DPMSolverSampler
    m = _model()
    cond, uc = conds()
    x0, mask = torch.zeros(SHAPE), mask_of("left")
    for s in (_sampler(m), _sampler(m, 0.0, DPMSolverSampler)):
        eta = 0.0 if isinstance(s, DPMSolverSampler) else 1.0
        sample = lambda **kw: s.sample(S, 1, SHAPE[1:], cond, eta=eta, unconditional_guidance_scale=SCALE, unconditional_conditioning=uc, **kw)
        decode = lambda **kw: s.decode(torch.zeros(SHAPE), cond, T_START, SCALE, uc, **kw)
        for call in (sample, decode):
            with pytest.raises(ValueError, match="go together"):
                call(mask=mask)
            with pytest.raises(ValueError, match="go together"):
                call(x0=x0)
            with pytest.raises(ValueError, match="latents' shape"):
                call(mask=mask, x0=x0[:, :, :4])
            with pytest.raises(ValueError, match="broadcast"):
                call(mask=torch.ones(1, 1, 1, 16, 8), x0=x0)
            with pytest.raises(ValueError, match="broadcast"):
                call(mask=torch.ones(1, 1, 1, 4, 8, 16, 16), x0=x0)


def test_dpm_solver_still_refuses_step_noises():
    from moca_video_amd.sampler import DPMSolverSampler
    m = _model()
    cond, uc = conds()
    s = _sampler(m, 0.0, DPMSolverSampler)
    zeros = [torch.zeros(SHAPE)] * S
    with pytest.raises(ValueError, match="draws nothing"):
        s.sample(S, 1, SHAPE[1:], cond, noises=zeros)
    with pytest.raises(ValueError, match="draws nothing"):
        s.sample(S, 1, SHAPE[1:], cond, noises=zeros, mask=mask_of("left"), x0=torch.zeros(SHAPE), mask_noises=zeros)
    with pytest.raises(ValueError, match="draws nothing"):
        s.decode(torch.zeros(SHAPE), cond, T_START, noises=zeros, mask=mask_of("left"), x0=torch.zeros(SHAPE))


def test_pixel_mask_is_min_pooled_to_latent_cells():
    from moca_video_amd.fifo import latent_mask
    lat = (1, 4, 2, 3, 5)
    px = torch.ones(1, 1, 2, 24, 40)
    px[0, 0, 0, 8 + 7, 16 + 7] = 0.0                        # cell (1, 2) of frame 0: 63 of its 64 pixels kept
    px[0, 0, 1, 0:8, 32:40] = 0.0                            # cell (0, 4) of frame 1: none kept
    got = latent_mask(px, lat)
    want = torch.ones(1, 1, 2, 3, 5)
    want[0, 0, 0, 1, 2] = 0.0
    want[0, 0, 1, 0, 4] = 0.0
    assert got.shape == want.shape and torch.equal(got, want)
    assert torch.equal(latent_mask(px[0, 0, 0], lat), want[0, 0, 0])                # fewer leading dims: the same cells
    at_latent = torch.rand(1, 1, 2, 3, 5)
    assert latent_mask(at_latent, lat) is at_latent                                  # latent resolution goes through as it is
    with pytest.raises(ValueError, match="neither"):
        latent_mask(torch.ones(1, 1, 2, 12, 20), lat)


def test_blend_mode_of_the_ddpm_entry_refuses_bad_arguments_without_a_gpu():
    """the blend alone -- `moca_ddpm_step_f32` without eps, with mask, x0, noise_q, x and out: nulls, misaligned fp32 operands, sizes,
    `per % mask_inner` and unknown flag bits return MOCA_E_BADARG before any launch; no new symbol is exported for it"""
    from moca_video_amd import lib
    l = lib.load()
    assert not any("blend" in n for n in lib.SIGNATURES)
    P = lambda off=0: C.c_void_p(0x10000 + off)
    names = ("state", "x", "out", "eps_c", "eps_u", "noise", "x_recon", "mean", "mask", "x0", "noise_q", "coef", "t")

    def call(t_stride=8, B=2, n_tab=1000, per=225, mask_inner=0, flags=lib.MOCA_DDPM_SCALE, **ptrs):
        base = dict(state=None, x=P(), out=P(), eps_c=None, eps_u=None, noise=None, x_recon=None, mean=None, mask=P(), x0=P(), noise_q=P(),
                    coef=P(), t=P())
        base.update(ptrs)
        return l.moca_ddpm_step_f32(*[base[n] for n in names], t_stride, B, n_tab, per, mask_inner, 1.0, 1.0, flags, None)
    for n in ("x", "out", "x0", "noise_q", "coef", "t"):
        assert call(**{n: None}) == -1, n
    for n in ("x", "out", "mask", "x0", "noise_q", "coef"):
        assert call(**{n: P(2)}) == -1, n
    assert call(t=P(4)) == -1 and call(eps_u=P()) == -1 and call(x_recon=P()) == -1 and call(mean=P()) == -1
    assert call(B=0) == -1 and call(per=0) == -1 and call(n_tab=0) == -1 and call(t_stride=-1) == -1
    assert call(flags=16) == -1 and call(flags=-1) == -1
    c0 = lib.MOCA_DDPM_MASK_C0
    assert call(flags=c0, mask_inner=0) == -1 and call(flags=c0, mask_inner=-45) == -1 and call(flags=c0, mask_inner=100) == -1
    assert call(flags=c0 | lib.MOCA_DDPM_SCALE, mask_inner=226) == -1


def test_drivers_are_exported_and_freeinit_says_it_takes_no_mask():
    import inspect
    import moca_video_amd as M
    from moca_video_amd.sampler import DDIMSampler, DPMSolverSampler
    for name in ("inpaint_ddim_sampling", "inpaint_dpm_solver_sampling"):
        assert name in M.__all__ and callable(getattr(M, name))
    for cls in (DDIMSampler, DPMSolverSampler):
        for fn in (cls.sample, cls.decode):
            p = inspect.signature(fn).parameters
            assert all(p[n].default is None and p[n].kind is p[n].POSITIONAL_OR_KEYWORD for n in ("mask", "x0", "mask_noises")), fn
    assert "mask" not in inspect.signature(DDIMSampler.sample_freeinit).parameters and "out of scope" in DDIMSampler.sample_freeinit.__doc__
    p = inspect.signature(M.inpaint_ddim_sampling).parameters
    assert (p["ddim_steps"].default, p["ddim_eta"].default, p["t_start"].default, p["paste_back"].default, p["use_graph"].default) == \
        (50, 0., None, True, True)
    p = inspect.signature(M.inpaint_dpm_solver_sampling).parameters
    assert (p["steps"].default, p["order"].default, p["paste_back"].default) == (20, 2, True)
