"""CPU: DPM-Solver++(2M) on the sampler's schedule rows (`fifo_graph.dpmpp_tables`, `fifo_graph.DpmEngine`, `sampler.DPMSolverSampler`,
the drivers of fifo.py) against the restatements of tests/dpm_solver_ref.py:

  * the step tables equal the float64 restatement to fp32 rounding, with the identity row, the first-step and last-step rules;
  * a first-order step is the DDIM step at eta 0 (float64: 1e-12; fp32: 4 x the fp32 forms' own deviation from float64);
  * on a Gaussian model with a closed-form solution the 2M trajectory's error at 20 steps is under an eighth of first order's, and the
    second-order LAST step (no `lower_order_final`) is worse than the first-order one -- the reason for the default;
  * what the sampler and the drivers refuse;
  * `DpmEngine` and the host-issued loop on a plan that holds buffers only (the tracer of tests/sampler_routes_cpu.py): which launches
    run, with which flag word, how many forwards;
  * `DDIMSampler`'s routes are the parent commit's with the new class imported, and the library's symbols are what they were."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import dpm_solver_ref as D
import sampler_routes_cpu as R
from v2v_ref import ScheduleModel

F32, F64 = torch.float32, torch.float64
ULP = 2.0 ** -23


def dpm_sampler(S, use_scale=True, order=2, lower_order_final=True):
    from moca_video_amd.sampler import DPMSolverSampler
    m = ScheduleModel()
    m.use_scale = use_scale
    s = DPMSolverSampler(m, order=order, lower_order_final=lower_order_final)
    s.make_schedule(S, verbose=False)
    return s


# ---- tables ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_scale", [True, False])
@pytest.mark.parametrize("order,lof", [(1, True), (2, True), (2, False)])
@pytest.mark.parametrize("S,n_rows", [(1, 1), (2, 2), (3, 3), (10, 10), (20, 20), (10, 6), (20, 1), (20, 2)])
def test_tables_equal_the_restatement(S, n_rows, order, lof, use_scale):
    from moca_video_amd.fifo_graph import dpm_stepped_rows, dpmpp_tables
    s = dpm_sampler(S, use_scale)
    coef, t_table = dpmpp_tables(s, n_rows, order, lof)
    assert coef.dtype == F32 and tuple(coef.shape) == (n_rows, 8) and t_table.dtype == torch.int64
    assert t_table.tolist() == [int(t) for t in s.ddim_timesteps[:n_rows]]
    tab = D.tables64(*D.schedule64(s, n_rows), order, lof)
    ref = D.coef_table(tab)
    got = coef.numpy().astype(np.float64)
    # fp32 rounding: half an ulp for the one rounding of a float64 value; columns 0 and 3 are the DDIM step's own fp32 roots (one
    # more rounding).  One ulp covers both.
    worst = np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300))
    print(f"[tables] S={S} n_rows={n_rows} order={order} lof={lof} use_scale={use_scale}: worst |got - ref| / |ref| = {worst / ULP:.3f} ulp")
    assert np.all(np.abs(got - ref) <= ULP * np.abs(ref))
    assert np.all(got[:, 6:] == 0)
    # the identity row at i = 0 (ddim_timesteps[0] = 0, ddim_alphas_prev[0] = alphas_cumprod[0]); it is not stepped
    assert tab["h"][0] == 0 and tuple(got[0, [1, 2, 4]]) == (0.0, 0.0, 1.0)
    assert dpm_stepped_rows(coef) == len(tab["stepped"]) == n_rows - 1
    stepped = tab["stepped"]
    for k, i in enumerate(stepped):
        first, last = k == 0, k == len(stepped) - 1
        second = order == 2 and not first and not (lof and last)
        assert (got[i, 2] != 0) == second, f"row {i}: c_1 = {got[i, 2]}"
        assert got[i, 1] != 0 and got[i, 4] != 1
    if S <= 2 or n_rows <= 2:
        assert np.all(got[:, 2] == 0)                       # one stepped row at the most: no second-order row


def test_tables_refuse_what_they_cannot_serve():
    from moca_video_amd.fifo_graph import dpmpp_tables
    from moca_video_amd.sampler import DDIMSampler
    s = dpm_sampler(10)
    for bad in (0, 3, "2"):
        with pytest.raises(ValueError):
            dpmpp_tables(s, 10, bad, True)
    for bad in (0, 11):
        with pytest.raises(ValueError):
            dpmpp_tables(s, bad, 2, True)
    eta1 = DDIMSampler(ScheduleModel())
    eta1.make_schedule(10, ddim_eta=1.0, verbose=False)
    with pytest.raises(ValueError):
        dpmpp_tables(eta1, 10, 2, True)
    quad = dpm_sampler(10)
    quad.make_schedule(50, ddim_discretize="quad", verbose=False)          # repeated timesteps above the clean end
    assert len(set(quad.ddim_timesteps.tolist())) < 50
    with pytest.raises(ValueError):
        dpmpp_tables(quad, 50, 2, True)


# ---- first order is DDIM at eta 0 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_scale", [True, False])
def test_first_order_is_ddim_at_eta_0(use_scale):
    from moca_video_amd.fifo_graph import BaseEngine, dpmpp_tables
    S = 20
    s = dpm_sampler(S, use_scale, order=1)
    a, ap, sc, scp = D.schedule64(s)
    ref = D.coef_table(D.tables64(a, ap, sc, scp, 1, True))
    coef32, _ = dpmpp_tables(s, S, 1, True)
    ddim32, _ = BaseEngine._schedule_tables(s, S)
    g = torch.Generator().manual_seed(11)
    worst64 = dev_first = dev_ddim = diff32 = 0.0
    for i in range(S):
        x, eps = torch.randn(4096, generator=g, dtype=F64), torch.randn(4096, generator=g, dtype=F64)
        x64, p64 = D.step64(x, eps, None, ref[i], use_scale)
        xd64, pd64 = D.ddim_tail64(x, eps, a[i], ap[i], sc[i], scp[i], use_scale)
        assert torch.equal(p64, pd64)
        worst64 = max(worst64, float((x64 - xd64).abs().max() / xd64.abs().max()))
        x32, p32 = D.step32(x, eps, None, None, coef32[i], 1.0, use_scale)
        xd32, pd32 = D.ddim_tail32(x, eps, ddim32[i, :7], use_scale)
        assert torch.equal(p32, pd32), f"row {i}: pred_x0 is not DDIM's bit for bit"
        scale = float(xd64.abs().max())
        dev_first = max(dev_first, float((x32.to(F64) - x64).abs().max()) / scale)
        dev_ddim = max(dev_ddim, float((xd32.to(F64) - xd64).abs().max()) / scale)
        diff32 = max(diff32, float((x32.to(F64) - xd32.to(F64)).abs().max()) / scale)
    print(f"[first order = DDIM] use_scale={use_scale}: float64 {worst64:.3e}; fp32 first order vs float64 {dev_first:.3e}, fp32 DDIM vs "
          f"float64 {dev_ddim:.3e}, fp32 first order vs fp32 DDIM {diff32:.3e}")
    assert worst64 <= 1e-12
    assert diff32 <= 4 * max(dev_first, dev_ddim)


# ---- order of accuracy ----------------------------------------------------------------------------------------------------------
def gaussian_errors(S, sdev=2.0, n=4096, dtype=F64):
    s = dpm_sampler(S, use_scale=False)
    a, ap, sc, scp = D.schedule64(s)
    x_T = torch.randn(n, generator=torch.Generator().manual_seed(5), dtype=F64) * float(np.sqrt(a[-1] * sdev * sdev + 1 - a[-1]))
    exact = D.gaussian_exact(x_T, a[-1], ap[0], sdev)
    run = lambda order, lof: D.rel_err(D.gaussian_run(D.tables64(a, ap, sc, scp, order, lof), a, x_T, sdev, dtype), exact)
    return run(1, True), run(2, True), run(2, False)


@pytest.mark.parametrize("dtype", [F64, F32])
def test_second_order_beats_first_order_on_the_gaussian_model(dtype):
    e1, e2, e2_nolof = gaussian_errors(20, dtype=dtype)
    print(f"[gaussian] S=20 s=2 {dtype}: first order {e1:.3e}, 2M lower_order_final {e2:.3e}, 2M without {e2_nolof:.3e}")
    assert e2 < e1 / 8                                      # (3.88e-3 against 5.39e-2)
    assert e2_nolof > e2                                    # (1.76e-2: the second-order term over the last step's h of about 2 hurts)
    f1, f2, _ = gaussian_errors(10, dtype=dtype)
    print(f"[gaussian] S=10 s=2 {dtype}: first order {f1:.3e}, 2M lower_order_final {f2:.3e}")
    assert f2 < f1


def test_package_tables_reach_the_same_gaussian_error():
    """the package's fp32 tables, stepped by the kernel's restatement, on the Gaussian model"""
    from moca_video_amd.fifo_graph import dpm_stepped_rows, dpmpp_tables
    sdev = 2.0
    errs = {}
    for order in (1, 2):
        s = dpm_sampler(20, use_scale=False, order=order)
        a, ap, _, _ = D.schedule64(s)
        coef, _ = dpmpp_tables(s, 20, order, True)
        x_T = torch.randn(4096, generator=torch.Generator().manual_seed(5), dtype=F64) * float(np.sqrt(a[-1] * sdev * sdev + 1 - a[-1]))
        x, hist = x_T.to(F32), None
        for k in range(dpm_stepped_rows(coef)):
            i = 19 - k
            x, hist = D.step32(x, D.gaussian_eps(x.to(F64), a[i], sdev).to(F32), None, hist, coef[i], 1.0, False)
        errs[order] = D.rel_err(x, D.gaussian_exact(x_T, a[-1], ap[0], sdev))
    print(f"[gaussian] package tables: first order {errs[1]:.3e}, 2M {errs[2]:.3e}")
    assert errs[2] < errs[1] / 8


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_sampler_refusals():
    import types
    from moca_video_amd import DPMSolverSampler, dpm_solver_sampling, fifo_ddim_sampling_multiprompts, v2v_dpm_solver_sampling
    from moca_video_amd.fifo import fifo_ddim_sampling
    from moca_video_amd.sampler import DDIMSampler
    m = ScheduleModel()
    for bad in (0, 3, True, 2.5):
        with pytest.raises(ValueError):
            DPMSolverSampler(m, order=bad)
    s = DPMSolverSampler(m)
    assert isinstance(s, DDIMSampler) and s.order == 2 and s.lower_order_final is True
    with pytest.raises(ValueError):
        s.make_schedule(10, ddim_eta=1.0, verbose=False)
    x = torch.zeros(1, 4, 2, 2, 2)
    c = {"c_crossattn": [torch.zeros(1, 3, 8)]}
    with pytest.raises(ValueError):
        s.sample(10, 1, (4, 2, 2, 2), c, eta=0.5, x_T=x)
    with pytest.raises(ValueError):
        s.sample(10, 1, (4, 2, 2, 2), c, x_T=x, noises=[x] * 10)
    with pytest.raises(ValueError):
        s.sample(10, 1, (4, 2, 2, 2), c, x_T=x, temperature=0.5)
    s.make_schedule(10, verbose=False)
    with pytest.raises(ValueError):
        s.decode(x, c, 5, noises=[x] * 5)
    with pytest.raises(ValueError):
        s.sample_freeinit([2, 3], 1, (4, 2, 2, 2), torch.ones(1, 1, 2, 2, 2), c, x_T=x, noises=[[x] * 2, [x] * 3])
    with pytest.raises(ValueError):
        s.sample_freeinit([2, 3], 1, (4, 2, 2, 2), torch.ones(1, 1, 2, 2, 2), c, x_T=x, eta=1.0)
    with pytest.raises(ValueError):
        dpm_solver_sampling(m, c, (1, 4, 2, 2, 2), order=3)
    with pytest.raises(ValueError):
        v2v_dpm_solver_sampling(m, c, latents=x, steps=10, t_start=10)
    with pytest.raises(ValueError):
        v2v_dpm_solver_sampling(m, c, latents=x, frames=x)
    args = types.SimpleNamespace(num_inference_steps=4, video_length=2, num_partitions=2, lookahead_denoising=False, new_video_length=4)
    with pytest.raises(NotImplementedError, match="first-order"):
        fifo_ddim_sampling(args, m, c, (1, 4, 2, 2, 2), s)
    with pytest.raises(NotImplementedError, match="first-order"):
        fifo_ddim_sampling_multiprompts(args, m, c, (1, 4, 2, 2, 2), s, [])
    # what stays the parent's
    for name in ("p_sample_ddim", "ddim_step", "fifo_onestep", "encode", "stochastic_encode", "decode", "ddim_update", "unet"):
        assert getattr(DPMSolverSampler, name) is getattr(DDIMSampler, name), name
    import inspect
    for name in ("sample", "sample_freeinit", "make_schedule"):
        assert list(inspect.signature(getattr(DPMSolverSampler, name)).parameters) == list(inspect.signature(getattr(DDIMSampler, name)).parameters)


# ---- the engine and the host-issued loop on a plan that holds buffers only ---------------------------------------------------------
def _traced_sampler(trace, order=2, use_scale=True, S=R.S):
    from moca_video_amd.sampler import DPMSolverSampler
    m = R.make_model(trace, use_scale=use_scale)
    s = DPMSolverSampler(m, order=order)
    s.make_schedule(S, verbose=False)
    return m, s


@pytest.mark.parametrize("guided", [True, False])
def test_engine_launches(guided):
    from moca_video_amd.fifo_graph import BaseEngine, dpmpp_tables
    trace = []
    m, s = _traced_sampler(trace)
    c, uc = R._cond(R.EB, 3, 16, 1), R._cond(R.EB, 6, 16, 2) if guided else None
    x = R.grid(R.E_SHAPE, 3)
    with R.engine_tracing(trace) as fg:
        assert fg.DpmEngine.supported(m, R.cuda_like(x), c, uc, R.SCALE if guided else 1.0)
        assert fg.DpmEngine.supported(m, R.cuda_like(x), c, R._cond(R.EB, 6, 16, 2), 1.0)         # scale 1: one branch, uc unused
        assert not fg.DpmEngine.supported(m, x, c, uc, R.SCALE if guided else 1.0)               # host latents
        eng = fg.DpmEngine(m, s, x, c, uc, R.SCALE if guided else 1.0, n_rows=R.T_START)
        assert isinstance(eng, BaseEngine) and eng.guided == guided and eng.pred_x0 is not None
        assert eng.S == R.T_START and eng.n_stepped == R.T_START - 1
        assert torch.equal(eng.coef, dpmpp_tables(s, R.T_START, 2, True)[0])
        del trace[:]
        for _ in range(eng.n_stepped):
            eng.step()
        with pytest.raises(ValueError):
            eng.step()
        per_step = trace[:3]
        assert len(trace) == 3 * (R.T_START - 1) and trace[1::3] == ["forward"] * (R.T_START - 1)
        assert per_step[0].startswith("moca_base_set_timestep(") and per_step[2].startswith("moca_base_ddim_step_f32(")
        assert not any("randn" in line for line in trace)                                        # nothing is drawn
        args = per_step[2][len("moca_base_ddim_step_f32("):-1].split(",")
        assert (args[3] != "-") == guided                                                        # eps_u NULL without guidance
        assert args[5] != "-" and args[7] == str(R.T_START) and args[9] == "3"                   # the history; S; MULTISTEP | SCALE
        # a new trajectory on the same engine: the shorter schedule of a FreeInit iteration, then the engine's own again
        shorter = type(s)(m)
        shorter.make_schedule(4, verbose=False)
        eng.set_schedule(shorter)
        assert (eng.it0, eng.n_iter, eng.n_stepped) == (R.T_START - 4, R.T_START - 4, 3)
        assert torch.equal(eng.coef[:4], dpmpp_tables(shorter, 4, 2, True)[0])
        for _ in range(3):
            eng.step()
        with pytest.raises(ValueError):
            eng.step()
        eng.reinit(R.grid(R.E_SHAPE, 12), R.grid((1, 1, 2, 2, 2), 13), z_rand=R.grid(R.E_SHAPE, 14))
        assert eng.n_iter == eng.it0 and eng.n_stepped == 3
        eng.reset(x, c, uc)
        assert (eng.it0, eng.n_iter, eng.n_stepped) == (0, 0, R.T_START - 1)
        eng.encode(R.grid(R.E_SHAPE, 9), 3)
        eng.step()
        eng.close()


def test_engine_key_tells_what_the_capture_bakes_in():
    from moca_video_amd.fifo_graph import BaseEngine, DpmEngine
    trace = []
    m, s = _traced_sampler(trace)
    c, uc, x = R._cond(1, 3, 16, 1), R._cond(1, 3, 16, 2), R.grid((1, 4, 2, 2, 2), 3)
    k = DpmEngine.key(s, x, c, uc, R.SCALE)
    assert k[0] == "dpmpp" and k != BaseEngine.key(s, x, c, uc, R.SCALE)
    assert k == DpmEngine.key(s, R.grid((1, 4, 2, 2, 2), 4), c, uc, R.SCALE)
    assert DpmEngine.key(s, x, c, uc, 1.0) == DpmEngine.key(s, x, c, None, 1.0) != k
    assert DpmEngine.key(s, x, c, uc, R.SCALE, n_rows=4) != k
    for attr, other in (("order", 1), ("lower_order_final", False), ("use_scale", False)):
        saved = getattr(s, attr)
        setattr(s, attr, other)
        assert DpmEngine.key(s, x, c, uc, R.SCALE) != k, attr
        setattr(s, attr, saved)


@pytest.mark.parametrize("guided", [True, False])
def test_host_issued_loop_and_cache(guided):
    """`sample` host-issued: S - 1 guidance evaluations and as many step launches through the engine's entry point; with `use_graph`
    on a counting stand-in engine: one build, then resets, S - 1 steps each"""
    from moca_video_amd import sampler as SM
    trace, log = [], []
    m, s = _traced_sampler(trace)
    c, uc = R._cond(1, 3, 16, 1), R._cond(1, 3, 16, 2) if guided else None
    x = R.grid((1, 4, 2, 2, 2), 3)
    scale = R.SCALE if guided else 1.0
    s.use_graph = False
    with R.tracing(trace):
        out, _ = s.sample(R.S, 1, x.shape[1:], c, x_T=x, unconditional_guidance_scale=scale, unconditional_conditioning=uc)
    steps = [line for line in trace if line.startswith("moca_base_ddim_step_f32(")]
    assert len(steps) == R.S - 1 and all(line.split(",")[9] == "3" and line.split(",")[3] == "-" for line in steps)
    assert sum(line.startswith(("forward_segments(", "apply_model(")) for line in trace) == R.S - 1
    assert sum(line.startswith("moca_cfg_combine_f32(") for line in trace) == (R.S - 1 if guided else 0)
    assert not any(line.startswith("moca_ddim_update_f32(") for line in trace)
    assert out.shape == x.shape and out.data_ptr() != x.data_ptr()

    class Counting(R._counting(SM.DpmEngine, log)):
        n_stepped = property(lambda self: self.S - 1)

        def step(self):
            log.append("step")
    saved, SM.DpmEngine = SM.DpmEngine, Counting
    try:
        s.use_graph = True
        with R.tracing(trace):
            for _ in range(2):
                s.sample(R.S, 1, x.shape[1:], c, x_T=R.cuda_like(x), unconditional_guidance_scale=scale, unconditional_conditioning=uc)
            assert log.count("build") == 1 and log.count("reset") == 1 and log.count("step") == 2 * (R.S - 1)
            s.make_schedule(R.S, verbose=False)
            s.decode(R.cuda_like(x), c, R.T_START, unconditional_guidance_scale=scale, unconditional_conditioning=uc)
            assert log.count("build") == 2 and log.count("close") == 1 and log.count("step") == 2 * (R.S - 1) + R.T_START - 1
            del log[:]
            s.sample_freeinit([3, R.S], 1, x.shape[1:], R.grid((1, 1, 2, 2, 2), 13), c, x_T=R.cuda_like(x), z_rands=[x],
                              unconditional_guidance_scale=scale, unconditional_conditioning=uc)
            assert log.count("build") == 1 and log.count("step") >= 2
            s.release()
    finally:
        SM.DpmEngine = saved


# ---- what exists does not move ----------------------------------------------------------------------------------------------------
def test_ddim_sampler_routes_are_the_parents_with_the_new_class_imported():
    from moca_video_amd import DPMSolverSampler  # noqa: F401
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sampler_routes.npz")
    with np.load(gold) as z:
        parent = {k: z[k] for k in z.files}
    now = {}
    for which in ("sample", "decode"):
        for use_scale in (True, False):
            now[f"loop.{which}.eta0.use_scale{int(use_scale)}"] = R.trace_loop(which, 0.0, use_scale)
        now[f"loop.{which}.eta1.use_scale1"] = R.trace_loop(which, 1.0, True)
    for which in ("plain", "rows", "pred_x0", "adapter", "hybrid"):
        now[f"engine.base.{which}"] = R.trace_base_engine(which)
    now["engine.invert.unguided"] = R.trace_invert_engine("unguided")
    now["fifo.lookahead1.batch_windows1"] = R.trace_fifo(True, True)
    now["fifo.lookahead0.batch_windows0"] = R.trace_fifo(False, False)
    now["supported"] = R.supported_table()
    now["cache"] = R.cache_table()
    now["engine_errors"] = R.engine_errors()
    for k, v in now.items():
        assert list(v) == list(parent[k]), k
    tables = R.coefficient_tables()
    for k, v in tables.items():
        assert v.tobytes() == parent[k].tobytes(), k


def test_library_symbols_are_what_they_were():
    import small_kernels_ref as K
    import step_kernels_ref as SK
    from test_abi_cpu import header_symbols
    from moca_video_amd import lib
    assert set(lib.SIGNATURES) == set(K.LEDGER) | set(K.LEDGER_EXEMPT) == set(header_symbols())
    restype, argtypes = lib.SIGNATURES["moca_base_ddim_step_f32"]
    assert restype is C.c_int and len(argtypes) == len(SK.ENTRY["moca_base_ddim_step_f32"]) + 1        # (+ the stream)
    assert argtypes[9] is C.c_int32 and SK.ENTRY["moca_base_ddim_step_f32"][9] == "use_scale"
    assert (lib.MOCA_BASE_SCALE, lib.MOCA_BASE_MULTISTEP) == (D.SCALE_BIT, D.MULTISTEP) == (1, 2)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "moca_hip.h")).read()
    assert "#define MOCA_BASE_SCALE 1" in header and "#define MOCA_BASE_MULTISTEP 2" in header


def test_multistep_without_history_is_a_bad_argument():
    """the one new guard, answered before any launch (no GPU needed): bit 1 with pred_x0 NULL"""
    from moca_video_amd import lib
    l = lib.load()
    P = C.c_void_p(0x1000)
    call = lambda pred_x0, flags: l.moca_base_ddim_step_f32(P, P, P, None, P, pred_x0, P, 6, 1.0, flags, 256, None)
    assert call(None, D.MULTISTEP) == -1 and call(None, D.MULTISTEP | D.SCALE_BIT) == -1
    for drop in range(7):                                    # the old guards hold with the bit set
        if drop in (3, 5):
            continue
        a = [P, P, P, None, P, P, P]
        a[drop] = None
        assert l.moca_base_ddim_step_f32(*a, 6, 1.0, D.MULTISTEP, 256, None) == -1
    assert l.moca_base_ddim_step_f32(P, P, P, None, P, P, P, 0, 1.0, D.MULTISTEP, 256, None) == -1
    assert l.moca_base_ddim_step_f32(P, P, P, None, P, P, P, 6, 1.0, D.MULTISTEP, 0, None) == -1
