"""GPU: DDIM / DPM-Solver inpainting -- the blend-only mode of `moca_ddpm_step_f32`, the masked `BaseEngine` / `DpmEngine`, `sample` /
`decode` with `mask=` / `x0=` and the drivers `inpaint_ddim_sampling` / `inpaint_dpm_solver_sampling`, against goldens of the REAL
reference's `p_sample_ddim` / `q_sample` run in upstream's loop order (tests/golden/ddim_inpaint.npz,
tools/make_golden_ddim_inpaint.py) and against identities that need no golden.

Tolerances: the kernel, the engine against the host-issued loop, the zero-mask and the paste-back identities are bit-exact
(`torch.equal`).  Against the goldens the latents take the base loop's bound `TOL_BASE` (tests/test_loops_gpu.py: set for ten steps that
feed the fp16-storage UNet's output back in; the fixture has ten, `decode`'s six accumulate less).  The blend adds fp32 arithmetic
only and REPLACES part of the fed-back latents by values that do not depend on the UNet, so it cannot widen that error.  The tool
asserts that dropping the blend, q_sample at the neighbouring row and the DDPM order each move every case by more than 3 x TOL_BASE."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from ddim_inpaint_ref import CASES, S, SCALE, SHAPE, T_START, conds, mask_of, operands, torch_blend  # noqa: E402
from helpers import REDUCED, golden, inp, relerr, state_dict_for  # noqa: E402
from test_loops_gpu import TOL_BASE  # noqa: E402

UNET = {"target": "lvdm.modules.networks.openaimodel3d.UNetModel", "params": REDUCED}
SENT = 12345.0


def _dm(use_scale):
    from moca_video_amd import DenoiseModel
    m = DenoiseModel(UNET, use_scale=use_scale)
    m.model.diffusion_model.load_state_dict(state_dict_for(m.model.diffusion_model, 11), strict=True)
    return m.cuda()


@pytest.fixture(scope="module")
def dm():
    return _dm(True)


@pytest.fixture(scope="module")
def dm_noscale():
    return _dm(False)


@pytest.fixture(scope="module")
def cu():
    """loop_base's contexts and the named operands of the fixture, on the device, made once"""
    to = lambda v: [t.cuda() for t in v] if isinstance(v, list) else v.cuda()
    cond, uc = ({"c_crossattn": [c["c_crossattn"][0].cuda()], "fps": c["fps"].cuda()} for c in conds())
    return dict(cond=cond, uc=uc, ops={case: {k: to(v) for k, v in operands(case).items()} for case in CASES},
                masks={k: mask_of(k).cuda() for k in ("left", "frames")})


def _sampler(model, eta=1.0, use_graph=True, cls=None, rows=S):
    from moca_video_amd.sampler import DDIMSampler
    s = (cls or DDIMSampler)(model)
    s.use_graph = use_graph
    s.make_schedule(rows, ddim_eta=eta, verbose=False)
    return s


# ---- the kernel ---------------------------------------------------------------------------------------------------------------
def _launch_blend(x, x0, mask, nq, coef, t, B, per, inner, flags, t_stride=1):
    from moca_video_amd.ddpm import launch_ddpm_step
    launch_ddpm_step(coef, t, B=B, per=per, x=x, out=x, mask=mask, x0=x0, noise_q=nq, mask_inner=inner, flags=flags, t_stride=t_stride)


def _guarded(t, off):
    """a copy of `t` inside a buffer with 64 sentinel floats on each side, starting `off` floats past a 16-byte boundary"""
    n = t.numel()
    buf = torch.full((n + 132,), SENT, device="cuda")
    v = buf[64 + off:64 + off + n].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 * off
    return buf, v


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset_by_one_float"])
@pytest.mark.parametrize("shape,kind", [((2, 4, 1, 3, 5), "full"), ((2, 4, 1, 3, 5), "c0"), ((2, 3, 1, 3, 3), "full"), ((2, 3, 1, 3, 3), "c0"),
                                        ((2, 4, 1, 4, 5), "c0")],
                         ids=["per60_full", "per60_c0_inner15", "per27_full_straddle", "per27_c0_inner9_scalar", "per80_c0_inner20_vector"])
def test_blend_kernel_bit_equal_to_torch(shape, kind, off):
    """the blend alone (`moca_ddpm_step_f32` without eps, with a mask) == the fp32 torch expression, bit for bit, in place, over:
    per % 4 == 0 (4,1,3,5) and groups that straddle samples (3,1,3,3: per = 27); a full mask, a one-channel mask read element by
    element (inner 9, 15) and 16 bytes wide (inner 20); every pointer 16-byte aligned and every pointer one float past (the unaligned
    path); the scale bit on and off; the timestep rows of the first, a middle and the last table row, one per sample and (stride 0) one
    for both; mask values 0, 1 and 0.25.  64 sentinel floats on each side of x stay untouched.  m == 0 leaves x as it was, and on a
    clean row (sac 1, s1mac 0, scale 1) m == 1 gives x0 exactly."""
    from moca_video_amd import lib
    g = torch.Generator(device="cuda").manual_seed(11)
    r = lambda shp=shape: torch.randn(shp, device="cuda", generator=g)
    B, per = shape[0], shape[1] * shape[2] * shape[3] * shape[4]
    mshape = shape if kind == "full" else (B, 1) + shape[2:]
    inner = per if kind == "full" else per // shape[1]
    n_tab = 7
    coef = torch.rand(n_tab, 8, device="cuda", generator=g) + 0.1
    vals = torch.tensor([0.0, 1.0, 0.25], device="cuda")
    mask_mixed = vals[torch.randint(0, 3, mshape, device="cuda", generator=g)]
    x, x0, nq = r(), r(), r()
    bufs = [_guarded(t, off) for t in (x, x0, nq, mask_mixed)]
    (xbuf, xv), (_, x0v), (_, nqv), (_, mv) = bufs
    c0 = lib.MOCA_DDPM_MASK_C0 if kind == "c0" else 0
    zero = mask_mixed.expand(shape) == 0
    for use_scale in (False, True):
        for ts, stride in (([0, n_tab - 1], 1), ([3, 3], 1), ([n_tab - 1, 0], 0)):
            rows = [coef[ts[b * stride]].tolist() for b in range(B)]
            want = torch.cat([torch_blend(x[b:b + 1], x0[b:b + 1], mask_mixed[b:b + 1], nq[b:b + 1], rows[b][5], rows[b][6], rows[b][7], use_scale)
                              for b in range(B)])
            xv.copy_(x)
            _launch_blend(xv, x0v, mv, nqv, coef, torch.tensor(ts, device="cuda"), B, per, inner, c0 | (lib.MOCA_DDPM_SCALE if use_scale else 0),
                          stride)
            assert torch.equal(xv, want), (use_scale, ts, stride)
            assert bool((xbuf[:64 + off] == SENT).all() and (xbuf[64 + off + x.numel():] == SENT).all()), "the kernel wrote outside x"
            assert torch.equal(xv[zero], x[zero])
    row = coef[0].tolist()
    assert not torch.equal(torch_blend(x, x0, mask_mixed, nq, row[5], row[6], row[7], True), torch_blend(x, x0, mask_mixed, nq, row[5], row[6], row[7], False))
    # m == 0 everywhere: x is untouched, bit for bit; m == 1 on the clean row: x0, bit for bit
    clean = torch.tensor([[0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 1.0]], device="cuda")
    t0 = torch.zeros(1, dtype=torch.int64, device="cuda")
    for m, want in ((torch.zeros(mshape, device="cuda"), x), (torch.ones(mshape, device="cuda"), x0)):
        _, mv1 = _guarded(m, off)
        xv.copy_(x)
        _launch_blend(xv, x0v, mv1, nqv, clean if want is x0 else coef, t0, B, per, inner, c0 | lib.MOCA_DDPM_SCALE, 0)
        assert torch.equal(xv, want)


# ---- the engines against the host-issued loop ------------------------------------------------------------------------------------
def _two_prompts():
    fps = torch.tensor([10, 12]).cuda()
    cond = {"c_crossattn": [torch.cat([inp("loop.ctx1", (1, 77, 128)), inp("loop.ctx2", (1, 77, 128))]).cuda()], "fps": fps}
    uc = {"c_crossattn": [inp("loop.uctx", (1, 77, 128)).cuda().expand(2, -1, -1)], "fps": fps}
    return cond, uc


@pytest.mark.parametrize("solver", [False, True], ids=["BaseEngine", "DpmEngine"])
def test_engine_equals_host_issued_loop(dm, solver):
    """the masked one-graph step against the host-issued loop (`HostBlend` + the host-issued step), B = 2 prompts, 4 schedule rows, a
    one-channel mask: the same fixed noises / mask_noises give bit-equal latents at the end of `sample` on both paths, and after every
    step the engine, stepped by hand, holds what the host-issued blend + step make of the same latents (DDIM; the solver's host step
    carries a history, so there the per-step check is the timestep rows and the end result); a masked engine takes its draws together"""
    from moca_video_amd.sampler import DPMSolverSampler
    rows = 4
    g = torch.Generator(device="cuda").manual_seed(3)
    shape = (2,) + SHAPE[1:]
    r = lambda: torch.randn(shape, device="cuda", generator=g)
    x_T, x0 = r(), r()
    mask = (torch.rand((2, 1) + SHAPE[2:], device="cuda", generator=g) > 0.5).float()
    cond, uc = _two_prompts()
    noises, mnoises = [r() for _ in range(rows)], [r() for _ in range(rows)]
    sg = _sampler(dm, 0.0 if solver else 1.0, True, DPMSolverSampler if solver else None, rows)
    sh = _sampler(dm, 0.0 if solver else 1.0, False, DPMSolverSampler if solver else None, rows)
    draws = dict(mask_noises=mnoises) if solver else dict(noises=noises, mask_noises=mnoises)
    kw = dict(unconditional_guidance_scale=SCALE, unconditional_conditioning=uc, mask=mask, x0=x0)
    n_steps = rows - 1 if solver else rows                                       # (the solver does not step the identity row at t = 0)
    host, _ = sh.sample(rows, 2, shape[1:], cond, eta=0.0 if solver else 1.0, x_T=x_T, **kw, **draws)
    assert sh._base_engine is None
    got, _ = sg.sample(rows, 2, shape[1:], cond, eta=0.0 if solver else 1.0, x_T=x_T, **kw, **draws)
    eng = sg._base_engine[1]
    assert eng.masked and eng.plan.graph is not None and eng.n_iter - eng.it0 == n_steps
    print(f"[parity] masked {'DpmEngine' if solver else 'BaseEngine'} vs host-issued loop after {n_steps} steps: {relerr(got, host):.3e}")
    assert torch.equal(got, host) and torch.isfinite(got).all()
    # after every step: the engine stepped by hand against the host loop's step on the same latents
    from moca_video_amd.sampler import HostBlend
    eng.reset(x_T, cond, uc, 0, mask=mask, x0=x0)
    blend = HostBlend(dm, x_T, mask, x0)
    x = x_T.clone()
    for i in range(n_steps):
        t = int(sg.ddim_timesteps[rows - 1 - i])
        if solver:
            eng.step(mask_noise=mnoises[i])
        else:
            eng.step(noise=noises[i], mask_noise=mnoises[i])
        now = eng.latents()
        assert (eng.t_rows() == t).all()
        if not solver:                                                           # (the solver's host step needs its history: compared at the end above)
            xb = blend(x.clone(), t, mnoises[i])
            ts = torch.full((2,), t, device="cuda", dtype=torch.long)
            want, _ = sg.p_sample_ddim(xb, cond, ts, index=rows - 1 - i, unconditional_guidance_scale=SCALE, unconditional_conditioning=uc,
                                       noise=noises[i])
            assert torch.equal(now, want), f"step {i}"
        x = now
    assert torch.equal(x, got)
    with pytest.raises(ValueError):
        if solver:
            sg.sample(rows, 2, shape[1:], cond, x_T=x_T, noises=noises, **kw)    # `noises=` stays refused
        else:
            eng.step(noise=x)                                                    # both draws or neither
    sg.release()


# ---- against the real reference -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "host"])
@pytest.mark.parametrize("case", list(CASES))
def test_vs_reference_golden(dm, dm_noscale, cu, case, use_graph):
    """`sample` (cases a, b, d) and `decode` (case c) with the fixture's mask, x0 and named draws, on the step graph and host-issued,
    within TOL_BASE of max|ref| of the real reference's loop"""
    mask_name, eta, use_scale, n_rows = CASES[case]
    g = golden("ddim_inpaint")
    model = dm if use_scale else dm_noscale
    o = cu["ops"][case]
    s = _sampler(model, eta, use_graph)
    kw = dict(unconditional_guidance_scale=SCALE, unconditional_conditioning=cu["uc"], mask=cu["masks"][mask_name], x0=o["x0"],
              noises=o["noises"], mask_noises=o["mask_noises"])
    if n_rows == S:
        got, _ = s.sample(S, 1, SHAPE[1:], cu["cond"], eta=eta, x_T=o["x_T"], **kw)
    else:
        x_enc = s.stochastic_encode(o["x0"], torch.tensor([n_rows]), noise=o["enc_noise"])
        assert torch.equal(x_enc.cpu(), torch.from_numpy(g[case + "__x_enc"]))
        got = s.decode(x_enc, cu["cond"], n_rows, use_graph=use_graph, **kw)
    assert (s._base_engine is not None) == use_graph
    if use_graph:
        assert s._base_engine[1].masked and s._base_engine[1].S == n_rows and s._base_engine[0][-1] == ("c0" if mask_name == "left" else "full")
    e = relerr(got.cpu(), g[case])
    print(f"[parity] inpaint case {case} use_graph={use_graph}: {e:.3e} of max|ref| (bound {TOL_BASE:.1e})")
    assert e < TOL_BASE
    s.release()


# ---- identities that need no golden -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "host"])
def test_all_zero_mask_is_the_unmasked_sample(dm, cu, use_graph):
    o = cu["ops"]["a"]
    s = _sampler(dm, 1.0, use_graph)
    kw = dict(eta=1.0, x_T=o["x_T"], unconditional_guidance_scale=SCALE, unconditional_conditioning=cu["uc"], noises=o["noises"])
    plain, _ = s.sample(S, 1, SHAPE[1:], cu["cond"], **kw)
    zeros, _ = s.sample(S, 1, SHAPE[1:], cu["cond"], mask=torch.zeros_like(cu["masks"]["left"]), x0=o["x0"], mask_noises=o["mask_noises"], **kw)
    assert torch.equal(zeros, plain) and torch.isfinite(plain).all()
    masked, _ = s.sample(S, 1, SHAPE[1:], cu["cond"], mask=cu["masks"]["left"], x0=o["x0"], mask_noises=o["mask_noises"], **kw)
    assert relerr(masked, plain) > 3 * TOL_BASE                                  # the mask is not ignored
    s.release()


def test_masked_reset_reuses_the_graph(dm, cu):
    """a second masked call with ANOTHER mask of the same kind goes through `reset` on the cached engine -- no new capture, the same
    hipGraph handle -- and gives what a fresh engine gives; a mask of the other kind, or none, builds another engine"""
    o = cu["ops"]["a"]
    s = _sampler(dm, 1.0, True)
    kw = dict(eta=1.0, x_T=o["x_T"], unconditional_guidance_scale=SCALE, unconditional_conditioning=cu["uc"], x0=o["x0"], noises=o["noises"],
              mask_noises=o["mask_noises"])
    s.sample(S, 1, SHAPE[1:], cu["cond"], mask=cu["masks"]["left"], **kw)
    eng = s._base_engine[1]
    handle = eng.plan.graph.value
    other = torch.zeros(1, 1, 8, 16, 16, device="cuda")
    other[:, :, 2:5, 4:, :] = 1.0                                                # per-frame: still one channel
    again, _ = s.sample(S, 1, SHAPE[1:], cu["cond"], mask=other, **kw)
    assert s._base_engine[1] is eng and eng.plan.graph.value == handle, "another mask of the same kind must not capture again"
    fresh_s = _sampler(dm, 1.0, True)
    fresh, _ = fresh_s.sample(S, 1, SHAPE[1:], cu["cond"], mask=other, **kw)
    assert fresh_s._base_engine[1] is not eng and torch.equal(again, fresh)
    fresh_s.release()
    s.sample(S, 1, SHAPE[1:], cu["cond"], mask=cu["masks"]["frames"], **kw)
    assert s._base_engine[1] is not eng and s._base_engine[1].masked
    with pytest.raises(ValueError):
        s._base_engine[1].reset(o["x_T"], cu["cond"], cu["uc"], 0)                # a masked engine wants its mask and x0
    s.release()


@pytest.mark.parametrize("solver", [False, True], ids=["BaseEngine", "DpmEngine"])
def test_unmasked_engine_records_what_it_recorded(dm, cu, solver, monkeypatch):
    """the recorded step list of an unmasked engine: as many plan steps as a masked one's (the blend rides in `pre`), and in front of
    and behind the forward exactly the launches from before there was a mask -- [timestep rows, Philox draw (DDIM only)] ... [step];
    the masked engine adds one blend launch behind the draw (and, on the solver, the draw itself) and nothing else"""
    from moca_video_amd import lib
    from moca_video_amd.fifo_graph import BaseEngine, DpmEngine
    from moca_video_amd.sampler import DPMSolverSampler
    l = lib.load()
    log = []
    for name in ("moca_base_set_timestep", "moca_fifo_randn_f32", "moca_base_ddim_step_f32", "moca_ddim_update_f32", "moca_ddpm_step_f32",
                 "moca_q_sample_f32", "moca_cfg_combine_f32"):
        real = getattr(l, name)
        monkeypatch.setattr(l, name, (lambda real, name: lambda *a: log.append(name) or real(*a))(real, name))
    o = cu["ops"]["a"]
    s = _sampler(dm, 0.0 if solver else 1.0, True, DPMSolverSampler if solver else None)
    cls = DpmEngine if solver else BaseEngine
    before = ["moca_base_set_timestep"] + ([] if solver else ["moca_fifo_randn_f32"]) + ["moca_base_ddim_step_f32"]
    recorded = {}
    for masked in (False, True):
        kw = dict(mask=cu["masks"]["left"], x0=o["x0"]) if masked else {}
        eng = cls(dm, s, o["x_T"], cu["cond"], cu["uc"], SCALE, **kw)
        del log[:]
        eng.step()                                                               # the first step runs the recorded sequence eagerly
        eng.sync_to()
        torch.cuda.synchronize()
        recorded[masked] = (len(eng.plan.steps), list(log))
        eng.close()
    assert recorded[False][1] == before
    assert recorded[True][1] == ["moca_base_set_timestep", "moca_fifo_randn_f32", "moca_ddpm_step_f32", "moca_base_ddim_step_f32"]
    assert recorded[False][0] == recorded[True][0]


# ---- the drivers --------------------------------------------------------------------------------------------------------------
def test_driver_pastes_back_and_returns_the_golden_without(dm, cu):
    """`inpaint_ddim_sampling`: with paste_back the kept region of the returned latents IS x0, bit for bit, and the rest is finite and
    what the sampler returned; without it the driver returns the golden of case (a); a pixel-resolution mask is reduced to the same
    latent mask; `t_start` takes the v2v path"""
    from moca_video_amd import inpaint_ddim_sampling
    o, g = cu["ops"]["a"], golden("ddim_inpaint")
    mask = cu["masks"]["left"]
    kw = dict(latents=o["x0"], ddim_steps=S, ddim_eta=1.0, cfg_scale=SCALE, uc_emb=cu["uc"]["c_crossattn"][0], x_T=o["x_T"], noises=o["noises"],
              mask_noises=o["mask_noises"])
    images, sampler, raw = inpaint_ddim_sampling(dm, cu["cond"], mask, paste_back=False, **kw)
    assert images is None and sampler._base_engine is None
    e = relerr(raw.cpu(), g["a"])
    print(f"[parity] inpaint_ddim_sampling paste_back=False vs case a: {e:.3e} (bound {TOL_BASE:.1e})")
    assert e < TOL_BASE
    _, _, pasted = inpaint_ddim_sampling(dm, cu["cond"], mask, **kw)
    keep = mask.expand(SHAPE) == 1
    assert torch.equal(pasted[keep], o["x0"][keep]) and not torch.equal(raw[keep], o["x0"][keep])
    assert torch.equal(pasted[~keep], raw[~keep]) and torch.isfinite(pasted).all()
    px = mask.repeat_interleave(8, -2).repeat_interleave(8, -1)                   # [1,1,1,128,128]
    _, _, from_px = inpaint_ddim_sampling(dm, cu["cond"], px, **kw)
    assert torch.equal(from_px, pasted)
    oc = cu["ops"]["c"]
    _, _, v2v = inpaint_ddim_sampling(dm, cu["cond"], mask, t_start=T_START, paste_back=False, noise=oc["enc_noise"],
                                      **dict(kw, noises=oc["noises"], mask_noises=oc["mask_noises"], x_T=None))
    assert relerr(v2v.cpu(), g["c"]) < TOL_BASE
    with pytest.raises(ValueError):
        inpaint_ddim_sampling(dm, cu["cond"], mask, **dict(kw, latents=None))
    with pytest.raises(ValueError):
        inpaint_ddim_sampling(dm, cu["cond"], mask, t_start=S, **kw)


def test_solver_driver_graph_equals_host_and_the_mask_matters(dm, cu):
    """`inpaint_dpm_solver_sampling` over 20 rows (19 forwards): bit-equal between the graph and the host-issued path under fixed
    q-noises, the kept region pasted back exactly, and outside the tolerance of its own unmasked run"""
    from moca_video_amd import dpm_solver_sampling, inpaint_dpm_solver_sampling
    o = cu["ops"]["a"]
    mask = cu["masks"]["left"]
    mn = [inp(f"inpaint.solver.mnoise{k}", SHAPE).cuda() for k in range(19)]
    kw = dict(latents=o["x0"], steps=20, cfg_scale=SCALE, uc_emb=cu["uc"]["c_crossattn"][0], x_T=o["x_T"], mask_noises=mn)
    _, _, a = inpaint_dpm_solver_sampling(dm, cu["cond"], mask, use_graph=True, **kw)
    _, _, b = inpaint_dpm_solver_sampling(dm, cu["cond"], mask, use_graph=False, **kw)
    assert torch.equal(a, b) and torch.isfinite(a).all()
    keep = mask.expand(SHAPE) == 1
    assert torch.equal(a[keep], o["x0"][keep])
    _, _, plain = dpm_solver_sampling(dm, cu["cond"], SHAPE, steps=20, cfg_scale=SCALE, uc_emb=cu["uc"]["c_crossattn"][0], x_T=o["x_T"])
    assert relerr(a[~keep], plain[~keep]) > 3 * TOL_BASE
