"""GPU: FreeInit sampling (`moca_video_amd.fifo.freeinit_ddim_sampling`, `DDIMSampler.sample_freeinit`, `BaseEngine.reinit` /
`set_schedule`, `freeinit.freeinit_reinit`) against goldens of the REAL reference's q_sample / freq_mix_3d / DDIMSampler.sample
(tools/make_golden_freeinit.py).

Bounds, none of them set from what this code gives:
  * the re-initialisation alone: FREEINIT_TOL = 2e-5 of max|ref| (tests/small_kernels_ref.py: the bound of the fp32 DFT mix; the
    q_sample in front of it is two fp32 multiply-adds);
  * the device-resident re-initialisation against the host-composed one, a shorter schedule on a captured engine against a fresh
    engine, num_iters = 1 against base_ddim_sampling: bit for bit (the same kernels on the same operands);
  * every iteration of a trajectory: TOL_BASE = 1.7e-2 (tests/test_loops_gpu.py: set for ten guided steps; an iteration here has at
    most six, and the previous iteration's samples re-enter scaled by sqrt(alphas_cumprod[999]) ~ 0.07 and low-passed)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import REDUCED, golden, inp, relerr, state_dict_for  # noqa: E402
from small_kernels_ref import FREEINIT_TOL  # noqa: E402
from test_loops_gpu import TOL_BASE, VAE_DD  # noqa: E402

SHAPE_A, SHAPE_B = (1, 4, 8, 16, 16), (2, 4, 16, 16, 24)
FILTERS = ("gaussian", "butterworth", "ideal", "box")
UNET = "lvdm.modules.networks.openaimodel3d.UNetModel"
STEPS, ITERS, SCALE = 6, 3, 12.0


@pytest.fixture(scope="module")
def dm():
    """the model of tests/test_loops_gpu.py: reduced-width UNet (weights seed 11), reduced-width VAE (seed 5), use_scale"""
    from moca_video_amd import DenoiseModel
    m = DenoiseModel({"target": UNET, "params": REDUCED},
                     first_stage_config={"target": "lvdm.models.autoencoder.AutoencoderKL",
                                         "params": {"embed_dim": 4, "ddconfig": VAE_DD, "lossconfig": {"target": "torch.nn.Identity"}}},
                     scale_factor=0.18215)
    m.model.diffusion_model.load_state_dict(state_dict_for(m.model.diffusion_model, 11), strict=True)
    m.first_stage_model.load_state_dict(state_dict_for(m.first_stage_model, 5), strict=True)
    return m.cuda()


@pytest.fixture(scope="module")
def dm_noscale():
    """a `use_scale=False` model for the re-initialisation alone (its UNet is never run: no weights loaded)"""
    from moca_video_amd import DenoiseModel
    return DenoiseModel({"target": UNET, "params": REDUCED}, use_scale=False).cuda()


def _text():
    return {k: inp(n, (1, 77, 128)).cuda() for k, n in (("c1", "loop.ctx1"), ("uc", "loop.uctx"))}


def _loop_inputs():
    t = _text()
    cond = {"c_crossattn": [t["c1"]], "fps": torch.tensor([10]).cuda()}
    x_T = inp("freeinit.x_T", SHAPE_A).cuda()
    z_rands = [inp(f"freeinit.zrand{k}", SHAPE_A).cuda() for k in range(1, ITERS)]
    noises = [[inp(f"freeinit.noise{k}.{i}", SHAPE_A).cuda() for i in range(STEPS)] for k in range(ITERS)]
    return cond, t["uc"], x_T, z_rands, noises


def _lpf(shape, filter_type="butterworth"):
    from moca_video_amd.freeinit import get_freq_filter
    return get_freq_filter(shape, "cuda", filter_type, 4, 0.25, 0.25)


# ---- 5. the re-initialisation alone -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,tag,filter_type,use_scale",
                         [(f"A_{ft}", "A", ft, False) for ft in FILTERS] + [("A_butterworth_scale", "A", "butterworth", True),
                                                                            ("B_butterworth", "B", "butterworth", False)])
def test_freeinit_reinit_vs_reference_golden(dm, dm_noscale, key, tag, filter_type, use_scale):
    from moca_video_amd.freeinit import freeinit_reinit
    shape = SHAPE_A if tag == "A" else SHAPE_B
    z0, init, zr = (inp(f"freeinit.{n}.{tag}", shape).cuda() for n in ("z0", "init", "zrand"))
    got = freeinit_reinit(dm if use_scale else dm_noscale, z0, init, zr, _lpf(shape, filter_type))
    assert tuple(got.shape) == shape and got.dtype == torch.float32
    e = relerr(got.cpu(), golden("freeinit_reinit")[key])
    print(f"[parity] freeinit_reinit {key}: {e:.3e} of max|ref| (bound {FREEINIT_TOL:.0e})")
    assert e <= FREEINIT_TOL


# ---- 6. the engine's re-initialisation is the host's ----------------------------------------------------------------------------
def _engine(dm, steps=STEPS, seed=5):
    from moca_video_amd.fifo_graph import BaseEngine
    from moca_video_amd.sampler import DDIMSampler
    cond, uctx, x_T, _, _ = _loop_inputs()
    uc = dict(cond, c_crossattn=[uctx])
    s = DDIMSampler(dm)
    s.make_schedule(steps, ddim_eta=1.0, verbose=False)
    assert BaseEngine.supported(dm, x_T, cond, uc, SCALE)
    return BaseEngine(dm, s, x_T, cond, uc, SCALE, seed=seed), s, (x_T, cond, uc)


def test_engine_reinit_equals_host_reinit_bit_for_bit(dm):
    from moca_video_amd.freeinit import freeinit_reinit
    eng, _, (x_T, cond, uc) = _engine(dm)
    z0 = inp("freeinit.z0.A", SHAPE_A).cuda() * 40.0            # the size of a guided sample of this UNet
    init, zr, lpf = inp("freeinit.init.A", SHAPE_A).cuda(), inp("freeinit.zrand.A", SHAPE_A).cuda(), _lpf(SHAPE_A)
    try:
        eng.reset(z0, cond, uc, seed=5)
        eng.reinit(init, lpf, z_rand=zr, seed=6)
        got = eng.latents()
        assert torch.equal(got, freeinit_reinit(dm, z0, init, zr, lpf))
        # z_rand from the engine's own stream: the same seed gives the same latents on another engine, the next seed others
        eng2, _, _ = _engine(dm)
        try:
            def drawn(e, seed):
                e.reset(z0, cond, uc, seed=5)
                e.reinit(init, lpf, seed=seed)
                return e.latents()
            a, b, c = drawn(eng, 7), drawn(eng2, 7), drawn(eng, 8)
            assert torch.isfinite(a).all() and torch.equal(a, b) and not torch.equal(a, c)
            assert not torch.equal(a, got)
        finally:
            eng2.close()
    finally:
        eng.close()


# ---- 7. a shorter schedule on a captured engine ---------------------------------------------------------------------------------
def test_set_schedule_runs_a_shorter_schedule_without_a_new_capture(dm):
    from moca_video_amd.sampler import DDIMSampler
    eng, s6, (x_T, cond, uc) = _engine(dm, 6)
    noises = _loop_inputs()[4][0]
    try:
        for i in range(6):                                       # a whole 6-step trajectory: eager, capture, replays
            eng.step(noise=noises[i])
        full6 = eng.latents()
        graph, plan = eng.plan.graph, eng.plan
        assert graph is not None
        s4 = DDIMSampler(dm)
        s4.make_schedule(4, ddim_eta=1.0, verbose=False)
        eng.reset(x_T, cond, uc, seed=9)
        eng.set_schedule(s4)
        for i in range(4):
            eng.step(noise=noises[i])
        got = eng.latents()
        assert eng.plan is plan and eng.plan.graph is graph and eng.n_iter == 6
        fresh, _, _ = _engine(dm, 4)
        try:
            for i in range(4):
                fresh.step(noise=noises[i])
            ref = fresh.latents()
        finally:
            fresh.close()
        assert torch.isfinite(got).all() and torch.equal(got, ref)
        s7 = DDIMSampler(dm)
        s7.make_schedule(7, ddim_eta=1.0, verbose=False)
        with pytest.raises(ValueError):
            eng.set_schedule(s7)
        # `reset` puts the engine's own schedule back
        eng.reset(x_T, cond, uc, seed=9)
        for i in range(6):
            eng.step(noise=noises[i])
        assert torch.equal(eng.latents(), full6) and eng.plan.graph is graph
    finally:
        eng.close()


# ---- 8. the trajectory against the real reference -------------------------------------------------------------------------------
@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("mode", ["full", "fast"])
def test_freeinit_trajectory_vs_reference_golden(dm, mode, use_graph):
    from moca_video_amd import freeinit_ddim_sampling
    from moca_video_amd.fifo_graph import BaseEngine
    g = golden("freeinit_loop")
    cond, uctx, x_T, z_rands, noises = _loop_inputs()
    builds = []
    real_init = BaseEngine.__init__

    def counting(self, *a, **k):
        builds.append(1)
        real_init(self, *a, **k)
    BaseEngine.__init__ = counting
    try:
        images, sampler, samples = freeinit_ddim_sampling(dm, cond, SHAPE_A, STEPS, 1.0, SCALE, uc_emb=uctx, num_iters=ITERS,
                                                          use_fast_sampling=mode == "fast", x_T=x_T, z_rands=z_rands, noises=noises,
                                                          use_graph=use_graph, return_all=True)
    finally:
        BaseEngine.__init__ = real_init
    assert len(builds) == (1 if use_graph else 0), "the run builds (and captures) one engine, or none on the host-issued path"
    assert len(samples) == ITERS and images is not None and torch.isfinite(images).all()
    errs = [relerr(samples[k].cpu(), g[f"{mode}_samples{k}"]) for k in range(ITERS)]
    print(f"[parity] freeinit {mode} use_graph={use_graph}: per-iteration rel err " + ", ".join(f"{e:.3e}" for e in errs) +
          f" (bound {TOL_BASE:.1e})")
    for k, e in enumerate(errs):
        assert e < TOL_BASE, f"iteration {k}: samples rel err {e:.3e}"


# ---- 9. one iteration is base sampling ------------------------------------------------------------------------------------------
def test_one_iteration_is_base_ddim_sampling_bit_for_bit(dm):
    from moca_video_amd import freeinit_ddim_sampling
    from moca_video_amd.fifo import base_ddim_sampling
    cond, uctx, x_T, _, noises = _loop_inputs()
    _, _, ref = base_ddim_sampling(dm, cond, SHAPE_A, STEPS, 1.0, SCALE, uc_emb=uctx, x_T=x_T, noises=noises[0])
    img, _, got = freeinit_ddim_sampling(dm, cond, SHAPE_A, STEPS, 1.0, SCALE, uc_emb=uctx, num_iters=1, x_T=x_T, noises=noises[:1])
    assert torch.isfinite(got).all() and torch.equal(got, ref) and img is not None


# ---- 10. the other conditionings of the step graph ------------------------------------------------------------------------------
def _graph_vs_host(model, cond, uctx, shape, tag):
    """two coarse-to-fine iterations ([1, 3] steps), device-resident against host-composed, within TOL_BASE.  Measured: the
    image-attention model agrees to the bit; the hybrid stand-in 5.7e-8 after iteration 0 and 7.9e-3 after iteration 1 -- what
    `base_ddim_sampling` alone gives there between its two paths (5.2e-8 after one step, 7.6e-3 after two: they round the update in
    another order, and that 8-channel model under guidance 12 turns a 1e-7 change of x_T into 1e-2 within three steps)."""
    from moca_video_amd import freeinit_ddim_sampling
    x_T = inp(f"freeinit.{tag}.x_T", shape).cuda()
    z_rands = [inp(f"freeinit.{tag}.zrand1", shape).cuda()]
    noises = [[inp(f"freeinit.{tag}.noise{k}.{i}", shape).cuda() for i in range(3)] for k in range(2)]
    run = lambda ug: freeinit_ddim_sampling(model, cond, shape, 3, 1.0, SCALE, uc_emb=uctx, num_iters=2, use_fast_sampling=True, x_T=x_T,
                                            z_rands=z_rands, noises=noises, use_graph=ug, return_all=True)[2]
    on_graph, on_host = run(True), run(False)
    for k in range(2):
        e = relerr(on_graph[k].cpu(), on_host[k].cpu())
        print(f"[parity] freeinit {tag} iteration {k}: graph vs host-issued {e:.3e} (bound {TOL_BASE:.1e})")
        assert torch.isfinite(on_graph[k]).all() and e < TOL_BASE


def test_freeinit_with_image_tokens_graph_equals_host():
    from test_i2v_gpu import _lvd
    lvd = _lvd(True)
    shape = [1, 4, 8, 16, 16]
    cond = {"c_crossattn": [inp("i2v.loop.c93", (1, 93, 1024)).cuda()], "fps": torch.tensor([10]).cuda()}
    u77 = inp("i2v.loop.u77", (1, 77, 1024)).cuda()
    _graph_vs_host(lvd, cond, u77, shape, "i2v")


def test_freeinit_hybrid_graph_equals_host():
    from test_hybrid_gpu import _dm, _sample_inputs
    from moca_video_amd.fifo_graph import BaseEngine
    _, shape, cond, uctx, x_T, _ = _sample_inputs()
    dm8 = _dm(8, "hybrid")
    assert BaseEngine.supported(dm8, x_T, cond, dict(cond, c_crossattn=[uctx]), SCALE)
    _graph_vs_host(dm8, cond, uctx, shape, "hybrid")
