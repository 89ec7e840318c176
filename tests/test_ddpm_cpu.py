"""CPU: the host side of the DDPM sampler (moca_video_amd/ddpm.py) -- the posterior tables of `register_schedule` (ddpm3d.py:136-153)
against the real method's (tests/golden/ddpm_tables.npz, tools/make_golden_ddpm.py), the argument validation of
`moca_ddpm_step_f32`, the argument contracts of `p_sample_loop` (:634-636) and the cache key of the step graph."""
import ctypes as C

import numpy as np
import pytest
import torch

from ddpm_ref import FIX, LOOP_SHAPE, TABLE_NAMES, half_mask
from helpers import REDUCED, golden


def _model(**kw):
    from moca_video_amd import DenoiseModel
    return DenoiseModel({"target": "lvdm.modules.networks.openaimodel3d.UNetModel", "params": REDUCED}, **kw)


@pytest.fixture(scope="module")
def fix_model():
    return _model(**FIX)


def _ulps(a, b):
    a, b = (np.ascontiguousarray(v, dtype=np.float32).view(np.int32).astype(np.int64) for v in (a, b))
    return int(np.abs(a - b).max())


@pytest.mark.parametrize("tag,kw", [("default", {}), ("fix", FIX)])
def test_tables_equal_register_schedule(tag, kw):
    """float64 numpy rounded once, as the reference's `to_torch`: equal to 1 fp32 ulp (np.log may differ in the last float64 bit
    between hosts, which can move a rounding); read through the reference's attribute names; not part of the state_dict"""
    g = golden("ddpm_tables")
    m = _model(**kw)
    for n in TABLE_NAMES:
        got = getattr(m, n)
        ref = g[f"{tag}__{n}"]
        assert got.dtype == torch.float32 and tuple(got.shape) == ref.shape == (m.num_timesteps,)
        assert _ulps(got.numpy(), ref) <= 1, n
    assert not set(TABLE_NAMES) & set(m.state_dict()) and not set(TABLE_NAMES) & {k for k, _ in m.named_buffers()}
    assert m.v_posterior == 0. and m.log_every_t == 100 and m.clip_denoised is False
    assert _model(log_every_t=7, v_posterior=0.25).log_every_t == 7


def test_v_posterior_mixes_beta_into_the_variance():
    """:144-145: (1 - v) beta_tilde + v beta"""
    from moca_video_amd.ddpm import ddpm_tables
    from moca_video_amd.wrapper import make_beta_schedule
    betas = make_beta_schedule("linear", 8, linear_start=0.05, linear_end=0.6)
    a, b = ddpm_tables(betas), ddpm_tables(betas, v_posterior=1.0)
    assert a["posterior_variance"][0] == 0 and np.array_equal(b["posterior_variance"], betas.astype(np.float32))
    assert a["posterior_log_variance_clipped"][0] == np.float32(np.log(1e-20))


def test_coef_table_columns(fix_model):
    """coef[t] = {srac, srm1, c1, c2, std, sac, s1mac, scale}; std is exp(0.5 log variance) to an fp32 ulp of torch's"""
    t = fix_model._ddpm_host()
    coef = t["coef"]
    assert coef.shape == (8, 8) and coef.dtype == np.float32
    for j, n in ((0, "sqrt_recip_alphas_cumprod"), (1, "sqrt_recipm1_alphas_cumprod"), (2, "posterior_mean_coef1"), (3, "posterior_mean_coef2")):
        assert np.array_equal(coef[:, j], t[n])
    assert np.array_equal(coef[:, 5], fix_model.sqrt_alphas_cumprod.numpy())
    assert np.array_equal(coef[:, 6], fix_model.sqrt_one_minus_alphas_cumprod.numpy())
    assert np.array_equal(coef[:, 7], fix_model.scale_arr.numpy()[:8])
    std = (0.5 * torch.from_numpy(t["posterior_log_variance_clipped"])).exp().numpy()
    assert _ulps(coef[:, 4], std) <= 1
    assert np.array_equal(_model(**dict(FIX, use_scale=False))._ddpm_host()["coef"][:, 7], np.ones(8, np.float32))


def test_bad_arguments_are_rejected_without_a_gpu():
    """null / misaligned pointers and inconsistent operand sets return MOCA_E_BADARG before any launch"""
    from moca_video_amd import lib
    l = lib.load()
    P = lambda off=0: C.c_void_p(0x10000 + off)
    names = ("state", "x", "out", "eps_c", "eps_u", "noise", "x_recon", "mean", "mask", "x0", "noise_q", "coef", "t")

    def call(t_stride=1, B=2, n_tab=8, per=225, mask_inner=0, flags=0, **ptrs):
        base = dict(state=None, x=P(), out=P(), eps_c=P(), eps_u=None, noise=P(), x_recon=None, mean=None, mask=None, x0=None,
                    noise_q=None, coef=P(), t=P())
        base.update(ptrs)
        return l.moca_ddpm_step_f32(*[base[n] for n in names], t_stride, B, n_tab, per, mask_inner, 1.0, 1.0, flags, None)
    for n in ("x", "eps_c", "noise", "coef", "t"):
        assert call(**{n: None}) == -1, n                                           # a required operand is NULL
    for n in ("x", "out", "eps_c", "noise", "coef"):
        assert call(**{n: P(2)}) == -1, n                                           # fp32 operands: 4-byte aligned
    assert call(t=P(4)) == -1 and call(eps_u=P(1)) == -1 and call(state=P(2)) == -1
    assert call(B=0) == -1 and call(per=0) == -1 and call(n_tab=0) == -1 and call(t_stride=-1) == -1 and call(flags=16) == -1
    assert call(out=None) == -1                                                     # no output at all
    assert call(mask=P()) == -1 and call(x0=P(), noise_q=P()) == -1 and call(mask=P(), x0=P()) == -1      # the blend takes all three
    assert call(mask=P(), x0=P(), noise_q=P(), out=None, mean=P()) == -1            # ... and writes out
    assert call(mask=P(), x0=P(), noise_q=P(), flags=lib.MOCA_DDPM_MASK_C0, mask_inner=0) == -1
    assert call(mask=P(), x0=P(), noise_q=P(), flags=lib.MOCA_DDPM_MASK_C0, mask_inner=100) == -1          # 225 % 100 != 0
    assert call(eps_c=None, x=None, noise=None) == -1                               # q_sample only: needs x0, noise_q
    assert call(eps_c=None, x0=P(), noise_q=P(), mean=P()) == -1


def test_p_sample_loop_argument_contracts(fix_model):
    """:634-636 and the refused options, all before anything touches a GPU"""
    cond = torch.zeros(1, 77, 128)
    x0 = torch.zeros(LOOP_SHAPE)
    with pytest.raises(AssertionError):
        fix_model.p_sample_loop(cond, LOOP_SHAPE, mask=half_mask())
    with pytest.raises(AssertionError):
        fix_model.p_sample_loop(cond, LOOP_SHAPE, mask=half_mask()[:, :, :4], x0=x0)          # frame axis
    with pytest.raises(NotImplementedError):
        fix_model.p_sample_loop(cond, LOOP_SHAPE, noise_dropout=0.5)
    with pytest.raises(NotImplementedError):
        fix_model.p_sample(x0, cond, torch.tensor([3]), noise_dropout=0.5)
    with pytest.raises(NotImplementedError):
        fix_model.p_sample(x0, cond, torch.tensor([3]), score_corrector=object())
    with pytest.raises(ValueError):
        fix_model.q_sample(x0, torch.tensor([3]))                                             # no CPU path
    assert not hasattr(fix_model, "shorten_cond_schedule")


def test_engine_key_separates_what_the_graph_bakes_in():
    from moca_video_amd.ddpm import engine_key, mask_kind
    cond = {"c_crossattn": [torch.zeros(1, 77, 128)]}
    uc = {"c_crossattn": [torch.zeros(1, 77, 128)]}
    key = lambda shape=LOOP_SHAPE, c=cond, u=None, T=8, s=1.0, mask=None, clip=False, p="eps": engine_key(shape, c, u, T, s, mask, clip, p, "cuda:0")
    base = key()
    assert base == key()
    full = torch.ones(LOOP_SHAPE)
    others = [key(mask=half_mask()), key(mask=full), key(T=7), key(clip=True), key(u=uc, s=7.5), key(shape=(2,) + LOOP_SHAPE[1:]),
              key(c={"c_crossattn": [torch.zeros(1, 154, 128)]}), key(p="x0")]
    assert len(set(others + [base])) == len(others) + 1
    assert key(u=uc, s=7.5) != key(u=uc, s=2.0)
    assert mask_kind(half_mask(), LOOP_SHAPE) == "c0" and mask_kind(half_mask()[0], LOOP_SHAPE) == "c0" and mask_kind(full, LOOP_SHAPE) == "full"
