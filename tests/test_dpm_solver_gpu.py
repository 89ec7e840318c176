"""GPU: DPM-Solver++(2M) -- `multistep_step_kernel` of csrc/sampler.hip behind `moca_base_ddim_step_f32`'s flag word, `fifo_graph.DpmEngine`
and `sampler.DPMSolverSampler` -- against the restatements of tests/dpm_solver_ref.py.

Standard for the kernel: torch.equal with the fp32 restatement in the kernel's order of operations (the translation unit is built without
contraction), at n below / above a block and past the grid cap, at iter >= S, with eps_u NULL and not, with the scale bit on and off;
a first-order row must not read the history (NaN in it), a second-order row must.  Flag values 0 and 1 still give `base_eval` of
tests/step_kernels_ref.py.  On the Gaussian model the device trajectory meets the one-eighth condition of tests/test_dpm_solver_cpu.py.
The engine's trajectories equal the host-issued ones bit for bit (`sample` guided and unguided, `decode`, `sample_freeinit`), with one
replay fewer than schedule rows; first order agrees with `DDIMSampler.sample(eta=0)` under the CPU test's tolerance rule."""
import ctypes as C

import numpy as np
import pytest
import torch

import dpm_solver_ref as D
import step_kernels_ref as R

pytestmark = pytest.mark.gpu

from helpers import REDUCED, inp, state_dict_for  # noqa: E402
from test_step_kernels_gpu import SENT, Buffers, exact, launch, state_words  # noqa: E402
from moca_video_amd import lib as L  # noqa: E402
from moca_video_amd import ops  # noqa: E402

F32, F64 = torch.float32, torch.float64
CFG = R.BASE_CFG
SEED64 = 0x1234567_89abcdef


@pytest.fixture(autouse=True)
def _stream():
    ops.set_stream(None)
    yield
    torch.cuda.synchronize()


# ---- the kernel -----------------------------------------------------------------------------------------------------------------
def _kernel_inputs(S, n, seed):
    g = R.gen(seed)
    t = dict(x=torch.randn(n, generator=g), e_c=torch.randn(n, generator=g), e_u=torch.randn(n, generator=g), hist=torch.randn(n, generator=g),
             coef=0.3 + torch.rand(S, 8, generator=g))
    return t


def _launch_step(t, S, it, flags, eps_u, hist, coef=None):
    """one call on fresh buffers -> (x, history, state, buffers)"""
    b = Buffers()
    st = b.out("state", state_words(7, it, SEED64, 1))
    b.inp("eps_c", t["e_c"])
    b.inp("eps_u", t["e_u"] if eps_u else None)
    b.inp("coef", t["coef"] if coef is None else coef)
    b.inp("noise", torch.full_like(t["x"], float("nan")))                  # required, never read: NaN would show
    x = b.out("x", t["x"])
    h = b.out("pred_x0", hist)
    launch("moca_base_ddim_step_f32", b, S=S, cfg_scale=CFG, use_scale=flags, n=t["x"].numel())
    return x, h, st, b


@pytest.mark.parametrize("n", [1, 255, 257, R.WRAP])
@pytest.mark.parametrize("S,it", [(1, 0), (1, 1), (1, 5), (6, 0), (6, 5), (6, 6), (6, 15)])
def test_multistep_kernel_bit_for_bit(S, it, n):
    """iter in {0, S - 1, S, 2 S + 3} for S in {1, 6}"""
    t = _kernel_inputs(S, n, 7000 + 10 * S + it)
    row = R.schedule_row(it, S)
    first = t["coef"].clone()
    first[row, 2] = 0.0                                                     # the same table with this row first order
    nan_hist = torch.full((n,), float("nan"))
    want_state = torch.tensor([7, it + 1, 0x89abcdef - (1 << 32), 0x1234567, 0, 0, 0, 0], dtype=torch.int32)
    for eps_u in (True, False):
        for scale_bit in (1, 0):
            what = f"multistep S={S} iter={it} n={n} eps_u={int(eps_u)} scale={scale_bit}"
            flags = D.MULTISTEP | scale_bit
            e_u = t["e_u"] if eps_u else None
            # second order: the history is read, and rewritten
            x, h, st, b = _launch_step(t, S, it, flags, eps_u, t["hist"])
            want_x, want_p0 = D.step32(t["x"], t["e_c"], e_u, t["hist"], t["coef"][row], CFG, scale_bit)
            exact(x, want_x, what + " x (in place)")
            exact(h, want_p0, what + " history")
            exact(st, want_state, what + " state (iter + 1, ext_noise 0, head and seed untouched)")
            b.check(what)
            x0, _, _, _ = _launch_step(t, S, it, flags, eps_u, torch.zeros(n))
            assert not torch.equal(x0, x), what + ": a second-order row must read the history"
            # first order: NaN in the history reaches nothing, and is overwritten
            x, h, st, b = _launch_step(t, S, it, flags, eps_u, nan_hist, coef=first)
            want_x, want_p0 = D.step32(t["x"], t["e_c"], e_u, None, first[row], CFG, scale_bit)
            assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(h).all()), what + ": NaN history reached the outputs of a first-order row"
            exact(x, want_x, what + " first-order x")
            exact(h, want_p0, what + " first-order history")
            b.check(what + " first order")


def test_multistep_without_history_launches_nothing():
    t = _kernel_inputs(6, 257, 7100)
    b = Buffers()
    st = b.out("state", state_words(7, 2, SEED64, 1))
    for k_arg, k_in in (("eps_c", "e_c"), ("eps_u", "e_u"), ("coef", "coef"), ("noise", "hist")):
        b.inp(k_arg, t[k_in])
    x = b.out("x", t["x"])
    args = {a.lstrip("*"): None for a in R.ENTRY["moca_base_ddim_step_f32"]}
    for flags in (D.MULTISTEP, D.MULTISTEP | D.SCALE_BIT):
        args.update(S=6, cfg_scale=CFG, use_scale=flags, n=257, stream=C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert R.call(L, "moca_base_ddim_step_f32", args, b.ptr) == -1          # MOCA_E_BADARG
        torch.cuda.synchronize()
        exact(x, t["x"], "x after a refused call")
        exact(st, state_words(7, 2, SEED64, 1), "state after a refused call")
    b.check("refused call")


@pytest.mark.parametrize("name", ["s6_iter0_scale1_n257", "s6_iter_last_scale0_n255"])
def test_flag_values_0_and_1_are_the_ddim_step(name):
    """the flag word's old values: `base_step_kernel` still runs, column 7 of the table stays meaningless"""
    c = R.BASE_CASES[name]
    t = R.base_inputs(c)
    b = Buffers()
    b.out("state", state_words(7, c["iter"], SEED64, 1))
    for k_arg, k_in in (("eps_c", "e_c"), ("eps_u", "e_u"), ("noise", "noise"), ("coef", "coef")):
        b.inp(k_arg, t[k_in])
    x = b.out("x", t["x"])
    p0 = b.out("pred_x0", t["x"], SENT)
    launch("moca_base_ddim_step_f32", b, S=c["S"], cfg_scale=R.BASE_CFG, use_scale=c["use_scale"], n=c["n"])
    want_xp, want_p0 = R.base_eval(c, F32, t=t)
    exact(x, want_xp, f"flag {c['use_scale']} {name} x")
    exact(p0, want_p0, f"flag {c['use_scale']} {name} pred_x0")
    b.check(name)
    # and the same operands under the new bit give another answer: the multistep kernel reads the row as its own layout
    b2 = Buffers()
    b2.out("state", state_words(7, c["iter"], SEED64, 1))
    for k_arg, k_in in (("eps_c", "e_c"), ("eps_u", "e_u"), ("noise", "noise"), ("coef", "coef")):
        b2.inp(k_arg, t[k_in])
    x2 = b2.out("x", t["x"])
    b2.out("pred_x0", t["noise"])
    launch("moca_base_ddim_step_f32", b2, S=c["S"], cfg_scale=R.BASE_CFG, use_scale=c["use_scale"] | D.MULTISTEP, n=c["n"])
    row = t["coef"][R.schedule_row(c["iter"], c["S"])]
    want, _ = D.step32(t["x"], t["e_c"], t["e_u"], t["noise"], row, R.BASE_CFG, c["use_scale"])
    exact(x2, want, f"flag {c['use_scale'] | D.MULTISTEP} {name} x")
    assert not torch.equal(x2.cpu(), want_xp)


# ---- the Gaussian model on the device -------------------------------------------------------------------------------------------
def test_gaussian_model_on_the_device():
    """20 host-issued launches over the 20 rows (the identity row included: it must leave x as it is), eps from the closed form"""
    from moca_video_amd.fifo_graph import dpmpp_tables
    from moca_video_amd.sampler import DPMSolverSampler
    from v2v_ref import ScheduleModel
    sdev, S, n = 2.0, 20, 4096
    m = ScheduleModel()
    m.use_scale = False
    errs = {}
    for order in (1, 2):
        s = DPMSolverSampler(m, order=order)
        s.make_schedule(S, verbose=False)
        a, ap, _, _ = D.schedule64(s)
        coef = dpmpp_tables(s, S, order, True)[0].cuda()
        x_T = torch.randn(n, generator=torch.Generator().manual_seed(5), dtype=F64) * float(np.sqrt(a[-1] * sdev * sdev + 1 - a[-1]))
        x = x_T.to(F32).cuda()
        state = state_words(0, 0, 0, 0).cuda()
        hist = torch.full((n,), float("nan"), device="cuda")
        for k in range(S):
            i = S - 1 - k
            eps = D.gaussian_eps(x.to(F64), a[i], sdev).to(F32)
            before = x.clone()
            L.check(L.load().moca_base_ddim_step_f32(L.ptr(state), L.ptr(x), L.ptr(eps), None, L.ptr(x), L.ptr(hist), L.ptr(coef), S, 1.0,
                                                     D.MULTISTEP, n, C.c_void_p(torch.cuda.current_stream().cuda_stream)), "moca_base_ddim_step_f32")
            if i == 0:
                assert torch.equal(x, before), "the identity row moved x"
        assert int(state[1]) == S
        errs[order] = D.rel_err(x.cpu(), D.gaussian_exact(x_T, a[-1], ap[0], sdev))
    print(f"[gaussian, device] S=20 s=2: first order {errs[1]:.3e}, 2M {errs[2]:.3e}")
    assert errs[2] < errs[1] / 8


# ---- the engine against the host-issued loop --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dm():
    """the reduced-width UNet of tests/test_loops_gpu.py (weights seed 11), use_scale"""
    from moca_video_amd import DenoiseModel
    m = DenoiseModel({"target": "lvdm.modules.networks.openaimodel3d.UNetModel", "params": REDUCED})
    m.model.diffusion_model.load_state_dict(state_dict_for(m.model.diffusion_model, 11), strict=True)
    return m.cuda()


SHAPE = (2, 4, 8, 16, 16)
STEPS, SCALE = 6, 12.0


def _inputs():
    """the shapes of tests/test_loops_gpu.py::test_base_step_graph_equals_p_sample_ddim: B = 2 prompts, two fps"""
    t = {k: inp(n, (1, 77, 128)).cuda() for k, n in (("c1", "loop.ctx1"), ("c2", "loop.ctx2"), ("uc", "loop.uctx"))}
    x_T = torch.randn(SHAPE, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    fps = torch.tensor([10, 12]).cuda()
    cond = {"c_crossattn": [torch.cat([t["c1"], t["c2"]])], "fps": fps}
    uc = {"c_crossattn": [t["uc"].expand(2, -1, -1)], "fps": fps}
    return x_T, cond, uc


def _sampler(dm, use_graph, order=2):
    from moca_video_amd.sampler import DPMSolverSampler
    s = DPMSolverSampler(dm, order=order)
    s.use_graph = use_graph
    return s


@pytest.mark.parametrize("guided", [True, False])
def test_sample_engine_equals_host_issued(dm, guided):
    from moca_video_amd.fifo_graph import DpmEngine
    x_T, cond, uc = _inputs()
    kw = dict(unconditional_guidance_scale=SCALE, unconditional_conditioning=uc) if guided else {}
    sg, sh = _sampler(dm, True), _sampler(dm, False)
    try:
        assert DpmEngine.supported(dm, x_T, cond, uc if guided else None, SCALE if guided else 1.0)
        got, _ = sg.sample(STEPS, 2, SHAPE[1:], cond, x_T=x_T, **kw)
        key, eng = sg._base_engine
        assert isinstance(eng, DpmEngine) and key[0] == "dpmpp" and eng.guided == guided
        assert eng.n_iter == STEPS - 1 and eng.plan.n_runs == STEPS - 1 and eng.plan.graph is not None       # the identity row is skipped
        ref, _ = sh.sample(STEPS, 2, SHAPE[1:], cond, x_T=x_T, **kw)
        assert sh._base_engine is None
        assert got.shape == x_T.shape and bool(torch.isfinite(got).all()) and not torch.equal(got, x_T)
        assert torch.equal(got, ref), f"engine vs host-issued: {float((got - ref).abs().max()):.3e}"
        # a second `sample`: the cached engine, reset; whatever the history holds is not read; the same bits
        eng.sync_to()
        eng.pred_x0.fill_(float("nan"))
        again, _ = sg.sample(STEPS, 2, SHAPE[1:], cond, x_T=x_T, **kw)
        assert sg._base_engine[1] is eng and eng.plan.n_runs == 2 * (STEPS - 1)
        assert torch.equal(again, got)
        with pytest.raises(ValueError):
            eng.step()
    finally:
        sg.release()


def test_first_order_matches_ddim_at_eta_0(dm):
    """order 1 against `DDIMSampler.sample(eta=0)`: each trajectory's final latents against the float64 host loop over ITS OWN recorded
    eps, within 4 x the larger of the two fp32 restatement loops' deviation from that float64 loop (the tolerance rule of
    tests/test_dpm_solver_cpu.py); and the two float64 loops, the solver's and DDIM's, agree to 1e-12 over one eps sequence"""
    from moca_video_amd.fifo_graph import BaseEngine, dpmpp_tables
    from moca_video_amd.sampler import DDIMSampler
    x_T, cond, uc = _inputs()
    kw = dict(unconditional_guidance_scale=SCALE, unconditional_conditioning=uc)

    def recorded(s, **more):
        eps, inner = [], s._cfg_eps
        s._cfg_eps = lambda *a, **k: eps.append(inner(*a, **k)) or eps[-1]
        out, _ = s.sample(STEPS, 2, SHAPE[1:], cond, x_T=x_T, **kw, **more)
        return out.cpu(), [e.cpu() for e in eps]
    sd = _sampler(dm, False, order=1)
    got_dpm, eps_dpm = recorded(sd)
    ddim = DDIMSampler(dm)
    ddim.use_graph = False
    got_ddim, eps_ddim = recorded(ddim, eta=0.)
    assert len(eps_dpm) == STEPS - 1 and len(eps_ddim) == STEPS
    sg = _sampler(dm, True, order=1)
    try:
        on_engine, _ = sg.sample(STEPS, 2, SHAPE[1:], cond, x_T=x_T, **kw)
        assert torch.equal(on_engine.cpu(), got_dpm)
    finally:
        sg.release()
    a, ap, sc, scp = D.schedule64(sd)
    ref = D.coef_table(D.tables64(a, ap, sc, scp, 1, True))
    coef32 = dpmpp_tables(sd, STEPS, 1, True)[0]
    ddim32 = BaseEngine._schedule_tables(ddim, STEPS)[0]
    x0 = x_T.cpu()

    def first_order(eps, dtype):
        x = x0.to(dtype)
        for k in range(STEPS - 1):
            i = STEPS - 1 - k
            x = D.step64(x, eps[k], None, ref[i], True)[0] if dtype == F64 else D.step32(x, eps[k], None, None, coef32[i], 1.0, True)[0]
        return x

    def ddim_loop(eps, dtype):
        x = x0.to(dtype)
        for k in range(STEPS):
            i = STEPS - 1 - k
            x = D.ddim_tail64(x, eps[k], a[i], ap[i], sc[i], scp[i], True)[0] if dtype == F64 else D.ddim_tail32(x, eps[k], ddim32[i, :7], True)[0]
        return x
    f64_dpm, f64_ddim = first_order(eps_dpm, F64), ddim_loop(eps_ddim, F64)
    dev = lambda x, r: float((x.to(F64) - r).abs().max() / r.abs().max())
    dev_first, dev_ddim = dev(first_order(eps_dpm, F32), f64_dpm), dev(ddim_loop(eps_ddim, F32), f64_ddim)
    tol = 4 * max(dev_first, dev_ddim)
    e_dpm, e_ddim = dev(got_dpm, f64_dpm), dev(got_ddim, f64_ddim)
    link = dev(first_order(eps_ddim, F64), f64_ddim)
    print(f"[order 1 = DDIM, device] fp32 restatement loops vs float64: first order {dev_first:.3e}, DDIM {dev_ddim:.3e} -> tolerance {tol:.3e}; "
          f"device vs float64: solver {e_dpm:.3e}, DDIM {e_ddim:.3e}; float64 first order vs float64 DDIM over DDIM's eps {link:.3e}; "
          f"the two device trajectories (each through its own UNet calls) {dev(got_dpm, got_ddim.to(F64)):.3e}")
    assert e_dpm <= tol and e_ddim <= tol
    assert link <= 1e-12


def test_decode_engine_equals_host_issued(dm):
    from moca_video_amd.fifo_graph import DpmEngine
    x_T, cond, uc = _inputs()
    sg, sh = _sampler(dm, True), _sampler(dm, False)
    try:
        outs = []
        for s in (sg, sh):
            s.make_schedule(STEPS, verbose=False)
            x = s.stochastic_encode(x_T * 0.5, torch.full((2,), 3, dtype=torch.long), noise=x_T.flip(0))
            outs.append(s.decode(x, cond, 3, unconditional_guidance_scale=SCALE, unconditional_conditioning=uc))
        eng = sg._base_engine[1]
        assert isinstance(eng, DpmEngine) and eng.S == 3 and eng.plan.n_runs == 2
        assert bool(torch.isfinite(outs[0]).all()) and torch.equal(outs[0], outs[1])
    finally:
        sg.release()


def test_freeinit_runs_on_one_engine_and_equals_the_host_loop(dm):
    from moca_video_amd.freeinit import get_freq_filter
    x_T, cond, uc = _inputs()
    lpf = get_freq_filter(SHAPE, "cuda", "butterworth", 4, 0.25, 0.25)
    z = [torch.randn(SHAPE, device="cuda", generator=torch.Generator(device="cuda").manual_seed(4))]
    kw = dict(conditioning=cond, x_T=x_T, z_rands=z, unconditional_guidance_scale=SCALE, unconditional_conditioning=uc, return_all=True)
    sg, sh = _sampler(dm, True), _sampler(dm, False)
    try:
        got, every = sg.sample_freeinit([3, STEPS], 2, SHAPE[1:], lpf, **kw)
        eng = sg._base_engine[1]
        graph = eng.plan.graph
        assert graph is not None and eng.S == STEPS and eng.plan.n_runs == 2 + (STEPS - 1)      # one engine, captured once: no second capture
        ref, every_ref = sh.sample_freeinit([3, STEPS], 2, SHAPE[1:], lpf, **kw)
        assert len(every) == len(every_ref) == 2
        for k in range(2):
            assert bool(torch.isfinite(every[k]).all()) and torch.equal(every[k], every_ref[k]), f"trajectory {k}"
        assert torch.equal(got, every[1])
    finally:
        sg.release()


def test_drivers(dm):
    from moca_video_amd import dpm_solver_sampling, v2v_dpm_solver_sampling
    x_T, cond, _ = _inputs()
    uc_emb = inp("loop.uctx", (1, 77, 128)).cuda().expand(2, -1, -1)
    outs = [dpm_solver_sampling(dm, cond, list(SHAPE), steps=4, cfg_scale=SCALE, uc_emb=uc_emb, x_T=x_T, use_graph=g) for g in (True, False)]
    assert outs[0][0] is None and outs[0][1]._base_engine is None and torch.equal(outs[0][2], outs[1][2])
    outs = [v2v_dpm_solver_sampling(dm, cond, latents=x_T * 0.5, steps=4, t_start=3, cfg_scale=SCALE, uc_emb=uc_emb, noise=x_T, use_graph=g)[2]
            for g in (True, False)]
    assert bool(torch.isfinite(outs[0]).all()) and torch.equal(outs[0], outs[1])
