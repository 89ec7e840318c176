"""CPU: the start-from-a-video surface of `DDIMSampler` (ddim.py:652-692,972-1032) -- the new C-ABI entry and its argument checks, the
reference's signatures, the refusals, and the index arithmetic of `decode` / `ddim_inversion` against lists recorded from the REAL
reference methods (tests/golden/v2v_cases.npz, tools/make_golden_v2v.py::index_cases)."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

from helpers import golden
from v2v_ref import REF_SIGNATURES, S, ScheduleModel


def test_library_exports_q_sample_and_rejects_bad_arguments():
    from moca_video_amd import lib
    l = lib.load()
    assert hasattr(l, "moca_q_sample_f32") and "moca_q_sample_f32" in lib.SIGNATURES
    p = C.c_void_p(64)                                   # never dereferenced: every call below is refused before a launch
    ok = [p, p, p, p, p, p, 2, 10, 945, None]
    for k in range(6):                                   # each pointer NULL in turn
        a = list(ok)
        a[k] = None
        assert l.moca_q_sample_f32(*a) == -1, f"pointer {k}"
    for k, bad in ((6, 0), (6, -1), (7, 0), (7, -3), (8, 0), (8, -945)):      # B, n_tab, per
        a = list(ok)
        a[k] = bad
        assert l.moca_q_sample_f32(*a) == -1, f"argument {k} = {bad}"


def test_signatures_start_with_the_references():
    from moca_video_amd.sampler import DDIMSampler
    for name, ref in REF_SIGNATURES.items():
        got = list(inspect.signature(getattr(DDIMSampler, name)).parameters)[1:]
        assert got[:len(ref)] == ref, f"{name}: {got}"
    sig = inspect.signature(DDIMSampler.decode).parameters
    assert "noises" in sig and "use_graph" in sig and "features_adapter" not in sig
    assert sig["unconditional_guidance_scale"].default == 1.0 and sig["use_original_steps"].default is False
    sig = inspect.signature(DDIMSampler.ddim_inversion).parameters
    assert sig["eta"].default == 1.0 and "noises" in sig and "anchor_noise" in sig
    from moca_video_amd import v2v_ddim_sampling
    assert list(inspect.signature(v2v_ddim_sampling).parameters) == [
        "model", "cond", "latents", "frames", "ddim_steps", "t_start", "ddim_eta", "cfg_scale", "uc_emb", "noise", "noises", "use_graph"]
    from moca_video_amd.fifo_graph import BaseEngine
    assert list(inspect.signature(BaseEngine.encode).parameters)[1:] == ["x0", "t_index", "noise"]


def _sampler():
    from moca_video_amd.sampler import DDIMSampler
    s = DDIMSampler(ScheduleModel())
    s.make_schedule(S, ddim_eta=1.0, verbose=False)
    return s


def test_refusals():
    s = _sampler()
    with pytest.raises(NotImplementedError, match=r"ddim\.py:325.*ddim\.py:352"):
        s.decode(torch.zeros(1, 4, 2, 2, 2), None, 6, use_original_steps=True)
    with pytest.raises(NotImplementedError):             # stays refused as it was
        s.p_sample_ddim(torch.zeros(1, 4, 2, 2, 2), None, torch.zeros(1, dtype=torch.long), 0, use_original_steps=True)
    with pytest.raises(ValueError, match="5 dimensions"):
        s.ddim_inversion(torch.zeros(1, 3, 8, 8), 10)


def test_driver_argument_checks():
    from moca_video_amd import v2v_ddim_sampling
    x = torch.zeros(1, 4, 2, 2, 2)
    for t_start in (0, 10):
        with pytest.raises(ValueError, match="t_start"):
            v2v_ddim_sampling(None, None, latents=x, ddim_steps=10, t_start=t_start)
    with pytest.raises(ValueError, match="exactly one"):
        v2v_ddim_sampling(None, None, latents=x, frames=x, ddim_steps=10, t_start=6)
    with pytest.raises(ValueError, match="exactly one"):
        v2v_ddim_sampling(None, None, ddim_steps=10, t_start=6)


@pytest.mark.parametrize("t_start", [1, 6, 10])
def test_decode_step_sequence_matches_the_reference(t_start):
    """the host-issued loop of `decode`: (timestep, schedule index) of every p_sample_ddim call, as the real `decode` issues them"""
    g = golden("v2v_cases")[f"decode_S{S}_t{t_start}"]
    s = _sampler()
    calls = []

    def spy(x, c, t, index, **kw):
        assert kw["use_original_steps"] is False and t.shape == (2,) and t.dtype == torch.long
        calls.append((int(t[0]), int(index)))
        return x, x
    s.p_sample_ddim = spy
    x = torch.zeros(2, 4, 2, 2, 2)
    assert s.decode(x, None, t_start, use_graph=False) is x
    assert calls == list(zip(g[0].tolist(), g[1].tolist())) and len(calls) == t_start
    # the truncated-table engine's rule (row t_start - 1 - i of the first t_start rows at step i) gives the same sequence
    assert [(int(s.ddim_timesteps[:t_start][t_start - 1 - i]), t_start - 1 - i) for i in range(t_start)] == calls


def test_inversion_frame_index_matches_the_reference():
    from moca_video_amd.sampler import DDIMSampler
    g = golden("v2v_cases")
    keys = [k for k in g.files if k.startswith("inversion_")]
    assert len(keys) == 5
    for k in keys:
        N, T = (int(v[1:]) for v in k.split("_")[1:])
        assert DDIMSampler.inversion_frame_index(N, T) == g[k].tolist(), k


def test_encode_tables_are_fp32_and_sized():
    s = _sampler()
    a, b = s.encode_tables()
    assert a.dtype == b.dtype == torch.float32 and a.shape == b.shape == (S,)
    a, b = s.encode_tables(use_original_steps=True)
    assert a.dtype == b.dtype == torch.float32 and a.shape == b.shape == (1000,)
    ac = s.model.alphas_cumprod.numpy()                  # np.sqrt of the fp32 buffer, as ddim.py:89-90 takes it
    assert np.array_equal(a.numpy(), np.sqrt(ac)) and np.array_equal(b.numpy(), np.sqrt(1. - ac))


def test_schedule_square_roots_do_not_depend_on_the_host():
    """`sqrt_f32` is the correctly rounded fp32 square root (float64 sqrt rounded once more is correctly rounded for fp32 arguments),
    whatever this host's torch gives; `encode_tables` and the queue coefficients of `prepare_latents` / `ddim_inversion` are taken
    with it"""
    from moca_video_amd.sampler import sqrt_f32
    s = _sampler()
    ac = s.model.alphas_cumprod
    for v in (ac, 1 - ac):
        assert torch.equal(sqrt_f32(v), torch.from_numpy(np.sqrt(v.numpy().astype(np.float64)).astype(np.float32)))
    al = torch.as_tensor(np.asarray(s.ddim_alphas), dtype=torch.float32)
    assert torch.equal(s.encode_tables()[0], sqrt_f32(al)) and sqrt_f32(al).dtype == torch.float32
