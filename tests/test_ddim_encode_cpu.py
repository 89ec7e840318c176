"""CPU: `DDIMSampler.encode`, the deterministic DDIM inversion -- its coefficient rows, step order, signature and refusals against
tests/golden/ddim_encode_cases.npz (tools/make_golden_ddim_encode.py: the REAL `p_sample_ddim` on a sampler copy with swapped tables),
and the oracle's `p_sample_ddim` composed over a swapped schedule against the golden's scripted step."""
import inspect

import numpy as np
import pytest
import torch

from helpers import golden, inp
from v2v_ref import S, ScheduleModel

# upstream's DDIMSampler.encode, parameter names after `self`, in order; `use_graph` is the project's own, as in `decode`
ENCODE_SIGNATURE = ["x0", "c", "t_enc", "use_original_steps", "return_intermediates", "unconditional_guidance_scale",
                    "unconditional_conditioning", "callback", "use_graph"]


def _sampler(n=S, use_scale=True):
    from moca_video_amd.sampler import DDIMSampler
    m = ScheduleModel()
    m.use_scale = use_scale
    s = DDIMSampler(m)
    s.make_schedule(n, ddim_eta=1.0, verbose=False)
    return s


@pytest.mark.parametrize("tag,n,use_scale", [("S10", 10, True), ("S50", 50, True), ("S10_noscale", 10, False)])
def test_invert_coef_rows_are_the_golden_rows_bit_for_bit(tag, n, use_scale):
    from moca_video_amd.fifo_graph import InvertEngine, invert_coef
    g = golden("ddim_encode_cases")[f"coef_{tag}"]
    s = _sampler(n, use_scale)
    rows = np.asarray([invert_coef(s, i) for i in range(n)])
    assert rows.dtype == np.float32 and rows.shape == g.shape == (n, 7)
    assert np.array_equal(rows.view(np.uint32), g.view(np.uint32))
    assert (rows[:, 2] == 0).all() and ((rows[:, 5:] == 1).all() or use_scale)
    # the step table: inversion row i is STORED at row n - 1 - i (the captured kernels read row n - 1 - iter), the timesteps with it
    coef, t_table = InvertEngine._schedule_tables(s)
    assert coef.shape == (n, 8) and coef.dtype == torch.float32 and t_table.dtype == torch.int64
    assert np.array_equal(coef.numpy()[::-1, :7].view(np.uint32), g.view(np.uint32)) and (coef[:, 7] == 0).all()
    assert t_table.tolist()[::-1] == [int(t) for t in s.ddim_timesteps]


def test_invert_coef_is_ddim_coef_with_the_levels_swapped():
    """going up from a_prev[i] to a_t[i] undoes what `ddim_coef` row i goes down at sigma 0: the roots of the two alphas change places;
    level a_next of step i is level a_cur of step i + 1"""
    from moca_video_amd.fifo_graph import ddim_coef, invert_coef
    s = _sampler()
    s.make_schedule(S, ddim_eta=0.0, verbose=False)
    for i in range(S):
        d, v = ddim_coef(s, i), invert_coef(s, i)
        assert d[0] == v[1] and d[1] == v[0] and d[2] == v[2] == 0 and d[3] == v[4]
        if i + 1 < S:
            assert invert_coef(s, i + 1)[0] == v[1] and invert_coef(s, i + 1)[5] == v[6]


@pytest.mark.parametrize("t_enc", [1, 6, 10])
def test_step_sequence_matches_the_reference(t_enc):
    """(timestep, level index) of every step: the host-issued loop, and the engine's reversed tables read at row S - 1 - iter"""
    from moca_video_amd.fifo_graph import InvertEngine
    g = golden("ddim_encode_cases")[f"encode_S{S}_t{t_enc}"]
    want = list(zip(g[0].tolist(), g[1].tolist()))
    s = _sampler()
    seen_t, seen_i = [], []

    def eps(x, t, c, uc, scale, **kw):
        assert t.shape == (2,) and t.dtype == torch.long and (t == t[0]).all()
        seen_t.append(int(t[0]))
        return x

    def update(x, e, i, zeros=None):
        assert zeros is not None and zeros.shape == x.shape and not zeros.any()
        seen_i.append(int(i))
        return x, x
    s._cfg_eps, s.invert_update = eps, update
    ticks = []
    inter = []
    s._encode_host(torch.zeros(2, 4, 2, 2, 2), None, t_enc, None, 1.0, inter, ticks.append)
    assert list(zip(seen_t, seen_i)) == want and len(want) == t_enc
    assert ticks == list(range(t_enc)) and len(inter) == t_enc
    _, t_table = InvertEngine._schedule_tables(s)
    assert [(int(t_table[S - 1 - it]), it) for it in range(t_enc)] == want


@pytest.mark.parametrize("tag", ["guided", "plain"])
def test_oracle_step_over_swapped_tables_reproduces_the_golden_step(tag):
    """`oracle.sampler_oracle.p_sample_ddim` over a schedule whose tables are swapped (alphas <-> alphas_prev, scales likewise, sigma 0,
    sqrt(1 - a) rebuilt from alphas_prev) IS the inversion step: the golden's scripted step, bit for bit, with the oracle's roots pinned
    to the correctly rounded ones the golden was made with; and the seven scalars it reads are `invert_coef`'s"""
    from moca_video_amd.fifo_graph import invert_coef
    from oracle import hostmath
    from oracle import sampler_oracle as SO
    g = golden("ddim_encode_cases")
    index, scale = int(g[f"step_{tag}_index"]), float(g[f"step_{tag}_scale"])
    sch = SO.make_schedule(SO.ddpm_buffers(), S, 0.0)
    sw = dict(sch, ddim_alphas=sch["ddim_alphas_prev"], ddim_alphas_prev=sch["ddim_alphas"], ddim_scale_arr=sch["ddim_scale_arr_prev"],
              ddim_scale_arr_prev=sch["ddim_scale_arr"], ddim_sigmas=np.zeros(S),
              ddim_sqrt_one_minus_alphas=np.sqrt(1. - np.asarray(sch["ddim_alphas_prev"])))
    f32 = np.float32
    args = np.asarray([v for k in ("ddim_alphas", "ddim_alphas_prev") for a in np.asarray(sch[k], np.float64)
                       for v in (f32(a), f32(1.) - f32(a))], np.float32)
    shape = (1, 4, 3, 5, 7)
    x, e_c, e_u = (inp(f"ddim_encode.step.{tag}.{k}", shape) for k in ("x", "ec", "eu"))
    if scale == 1.0:
        e_u = torch.zeros_like(e_c)                      # the reference makes ONE model call at scale 1: e = e_c (0 + 1 (e_c - 0) exactly)
    with hostmath.pinned({"sqrt": (args, np.sqrt(args)), "exp": (np.zeros(1, f32), np.ones(1, f32))}):
        x_next, pred_x0 = SO.p_sample_ddim(sw, x, e_c, e_u, scale, index, torch.zeros(shape))
    assert torch.equal(x_next, torch.from_numpy(g[f"step_{tag}_x_next"]))
    assert torch.equal(pred_x0, torch.from_numpy(g[f"step_{tag}_pred_x0"]))
    s = _sampler()
    c = invert_coef(s, index)
    want = (np.sqrt(f32(sw["ddim_alphas"][index])), np.sqrt(f32(sw["ddim_alphas_prev"][index])), f32(0),
            f32(sw["ddim_sqrt_one_minus_alphas"][index]), np.sqrt(f32(1.) - f32(sw["ddim_alphas_prev"][index])),
            f32(sw["ddim_scale_arr"][index]), f32(sw["ddim_scale_arr_prev"][index]))
    assert all(a == b and np.asarray(a).dtype == np.float32 for a, b in zip(c, want))


def test_encode_signature_is_upstreams():
    from moca_video_amd.sampler import DDIMSampler
    sig = inspect.signature(DDIMSampler.encode).parameters
    assert list(sig)[1:] == ENCODE_SIGNATURE
    assert sig["use_original_steps"].default is False and sig["return_intermediates"].default is None
    assert sig["unconditional_guidance_scale"].default == 1.0 and sig["unconditional_conditioning"].default is None
    assert sig["callback"].default is None and sig["use_graph"].default is None


def test_encode_refusals():
    s = _sampler()
    x = torch.zeros(1, 4, 2, 2, 2)
    for t_enc in (0, -1, S + 1):
        with pytest.raises(ValueError, match="t_enc"):
            s.encode(x, None, t_enc)
    with pytest.raises(NotImplementedError, match="use_original_steps"):
        s.encode(x, None, 6, use_original_steps=True)
    with pytest.raises(ValueError, match="cuda"):
        s.encode(x, None, 6)                              # x0 on the host


def test_new_keywords_default_to_the_behaviour_before():
    """`ddim_inversion` noises unless asked (`deterministic=False`); its deterministic mode wants `cond` and refuses `noises=`;
    `v2v_ddim_sampling` keeps its pinned parameters and the inversion driver stands beside it, without an encode draw to fix"""
    from moca_video_amd import v2v_ddim_sampling, v2v_invert_sampling
    from moca_video_amd.sampler import DDIMSampler
    sig = inspect.signature(DDIMSampler.ddim_inversion).parameters
    assert list(sig)[1:7] == ["frames", "num_inference_steps", "eta", "latents_dir", "noises", "anchor_noise"]
    assert list(sig)[7:] == ["deterministic", "cond", "unconditional_guidance_scale", "unconditional_conditioning"]
    assert sig["deterministic"].default is False and sig["cond"].default is None
    assert sig["unconditional_guidance_scale"].default == 1.0 and sig["unconditional_conditioning"].default is None
    s = _sampler()
    frames = torch.zeros(1, 3, 2, 8, 8)
    with pytest.raises(ValueError, match="cond"):
        s.ddim_inversion(frames, 10, deterministic=True)
    with pytest.raises(ValueError, match="noises"):
        s.ddim_inversion(frames, 10, deterministic=True, cond={"c_crossattn": [torch.zeros(1, 77, 128)]}, noises=[frames])
    a, b = inspect.signature(v2v_ddim_sampling).parameters, inspect.signature(v2v_invert_sampling).parameters
    assert "invert" not in a and "src_cond" not in a
    assert "noise" not in b and b["src_cond"].default is None and b["src_cfg_scale"].default == 1.0 and b["ddim_eta"].default == 0.0
    assert [k for k in a if k in b] == [k for k in a if k != "noise"]
    x = torch.zeros(1, 4, 2, 2, 2)
    for t_start in (0, 11):
        with pytest.raises(ValueError, match="t_start"):
            v2v_invert_sampling(None, None, latents=x, ddim_steps=10, t_start=t_start)
    with pytest.raises(ValueError, match="exactly one"):
        v2v_invert_sampling(None, None, latents=x, frames=x, ddim_steps=10, t_start=6)
    with pytest.raises(ValueError, match="exactly one"):
        v2v_invert_sampling(None, None, ddim_steps=10, t_start=6)
