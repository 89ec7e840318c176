"""CPU: the host side of FreeInit sampling (`moca_video_amd.fifo.freeinit_ddim_sampling`) and its fixtures.

  * `freeinit_steps` and the refusals of `freeinit_ddim_sampling`, which raise before any device work;
  * the goldens of tools/make_golden_freeinit.py (the REAL reference's q_sample / freq_mix_3d / DDIMSampler.sample) against an
    independent composition: `oracle.freeinit_oracle.freq_mix_3d` over the two-term q_sample formula in numpy, within FREEINIT_TOL
    (2e-5 of max|ref|, the project's bound for this mix);
  * the fixture separates: iteration 1 of the golden trajectory is far from the two stored wrong variants -- (a) re-noised with
    z_rand in place of the initial noise, (b) the filter applied without the fftshift;
  * the package exports the new entry point and still exactly the header's symbols (tests/test_abi_cpu.py and
    test_small_kernels_cpu.py::test_ledger check the ledger itself)."""
import types

import numpy as np
import pytest
import torch

from helpers import golden, inp
from small_kernels_ref import FREEINIT_TOL

TOL_BASE = 1.7e-2                 # tests/test_loops_gpu.py (a GPU module: not imported here)
SHAPE_A, SHAPE_B = (1, 4, 8, 16, 16), (2, 4, 16, 16, 24)
FILTERS = ("gaussian", "butterworth", "ideal", "box")


def relerr(got, ref):
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    return ((got - ref).abs().max() / ref.abs().max()).item()


def schedule_last():
    """sqrt(alphas_cumprod[999]), sqrt(1 - alphas_cumprod[999]) and scale_arr[999] of the YAML's schedule, rounded to fp32 as
    `register_schedule` rounds them"""
    betas = np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=np.float64) ** 2
    ac = np.cumprod(1. - betas)
    return np.float32(np.sqrt(ac[-1])), np.float32(np.sqrt(1. - ac[-1])), np.float32(0.7)


def oracle_reinit(z0, initial_noise, z_rand, filter_type, use_scale):
    from oracle import freeinit_oracle as FO
    a, b, s = schedule_last()
    z0, initial_noise = np.asarray(z0, np.float32), np.asarray(initial_noise, np.float32)
    z_T = a * z0 * s + b * initial_noise if use_scale else a * z0 + b * initial_noise
    lpf = FO.get_freq_filter(z0.shape, filter_type, 4, 0.25, 0.25)
    return FO.freq_mix_3d(torch.from_numpy(z_T), torch.as_tensor(z_rand), lpf).reshape(z0.shape)


def test_freeinit_steps():
    from moca_video_amd.freeinit import freeinit_steps
    assert freeinit_steps(50, 5, False) == [50] * 5
    assert freeinit_steps(50, 5, True) == [10, 20, 30, 40, 50]
    assert freeinit_steps(6, 3, True) == [2, 4, 6]
    s = freeinit_steps(3, 5, True)
    assert len(s) == 5 and min(s) >= 1 and s[-1] == 3 and max(s) == 3
    assert freeinit_steps(7, 1, True) == [7]
    with pytest.raises(ValueError):
        freeinit_steps(10, 0)


def test_refusals_come_before_any_device_work():
    """a model without a device, a UNet or a schedule: every refusal must be raised before one of them is touched"""
    from moca_video_amd import freeinit_ddim_sampling
    model = types.SimpleNamespace(device=torch.device("cpu"))
    cond = {"c_crossattn": [torch.zeros(1, 77, 128)]}
    z = torch.zeros(SHAPE_A)
    with pytest.raises(ValueError, match="num_iters"):
        freeinit_ddim_sampling(model, cond, SHAPE_A, num_iters=0)
    with pytest.raises(NotImplementedError):
        freeinit_ddim_sampling(model, cond, SHAPE_A, num_iters=2, filter_type="lanczos")
    with pytest.raises(ValueError, match="noise_shape"):
        freeinit_ddim_sampling(model, cond, SHAPE_A[1:], num_iters=2)
    with pytest.raises(ValueError, match="z_rands"):
        freeinit_ddim_sampling(model, cond, SHAPE_A, num_iters=3, z_rands=[z])
    with pytest.raises(ValueError, match="noises"):
        freeinit_ddim_sampling(model, cond, SHAPE_A, ddim_steps=2, num_iters=3, z_rands=[z, z], noises=[[z, z]] * 2)


@pytest.mark.parametrize("key,tag,filter_type,use_scale",
                         [(f"A_{ft}", "A", ft, False) for ft in FILTERS] + [("A_butterworth_scale", "A", "butterworth", True),
                                                                            ("B_butterworth", "B", "butterworth", False)])
def test_golden_reinit_equals_oracle_composition(key, tag, filter_type, use_scale):
    g = golden("freeinit_reinit")
    shape = SHAPE_A if tag == "A" else SHAPE_B
    z0, init, zr = (inp(f"freeinit.{n}.{tag}", shape) for n in ("z0", "init", "zrand"))
    ref = torch.from_numpy(g[key])
    assert tuple(ref.shape) == shape
    e = relerr(oracle_reinit(z0, init, zr, filter_type, use_scale), ref)
    print(f"[freeinit] golden {key} vs oracle composition: {e:.3e} of max|ref|")
    assert e <= FREEINIT_TOL


@pytest.mark.parametrize("mode", ["full", "fast"])
def test_golden_trajectory_starts_equal_oracle_composition(mode):
    """every re-initialised start of the golden trajectories is the oracle's composition over the previous golden samples"""
    from moca_video_amd.freeinit import freeinit_steps
    g = golden("freeinit_loop")
    assert g[f"{mode}_steps"].tolist() == freeinit_steps(6, 3, mode == "fast")
    init = inp("freeinit.x_T", SHAPE_A)
    for k in (1, 2):
        ref = torch.from_numpy(g[f"{mode}_x_T{k}"])
        e = relerr(oracle_reinit(g[f"{mode}_samples{k - 1}"], init, inp(f"freeinit.zrand{k}", SHAPE_A), "butterworth", True), ref)
        print(f"[freeinit] golden {mode} x_T{k} vs oracle composition: {e:.3e} of max|ref|")
        assert e <= FREEINIT_TOL


@pytest.mark.parametrize("wrong", ["a", "b"])
def test_fixture_separates_the_wrong_variants(wrong):
    g = golden("freeinit_loop")
    ex = relerr(g[f"full_x_T1_wrong_{wrong}"], g["full_x_T1"])
    es = relerr(g[f"full_samples1_wrong_{wrong}"], g["full_samples1"])
    print(f"[freeinit] wrong variant ({wrong}): x_T {ex:.3e}, samples {es:.3e} of max|ref|")
    assert ex > 10 * FREEINIT_TOL
    assert es > 10 * TOL_BASE
    # and the stored variants are what they claim to be: the oracle composition with the same mistake
    init, zr = inp("freeinit.x_T", SHAPE_A), inp("freeinit.zrand1", SHAPE_A)
    from oracle import freeinit_oracle as FO
    a, b, s = schedule_last()
    z_T = a * g["full_samples0"] * s + b * (zr if wrong == "a" else init).numpy()
    lpf = FO.get_freq_filter(SHAPE_A, "butterworth", 4, 0.25, 0.25)
    if wrong == "b":
        lpf = torch.fft.fftshift(lpf, dim=(-3, -2, -1))
    mine = FO.freq_mix_3d(torch.from_numpy(z_T), zr, lpf).reshape(SHAPE_A)
    assert relerr(mine, g[f"full_x_T1_wrong_{wrong}"]) <= FREEINIT_TOL


def test_package_exports():
    import moca_video_amd
    from moca_video_amd import lib
    assert "freeinit_ddim_sampling" in moca_video_amd.__all__ and callable(moca_video_amd.freeinit_ddim_sampling)
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "moca_hip.h")).read()
    declared = set(re.findall(r"\b(moca_[a-z0-9_]+)\s*\(", header))
    assert set(lib.SIGNATURES) == declared
