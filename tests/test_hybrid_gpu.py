"""GPU: hybrid conditioning (c_concat joined to the latent along the channel axis, ddpm3d.py:713-759) through the HIP path:
moca_ncthw_scatter_f16 alone, the wrapper cases against goldens of the REAL reference wrapper + UNet (tests/golden/hybrid_wrapper.npz,
tools/make_golden_hybrid.py), bit-equality with the plain forward of the materialised concat, the untouched in_channels = 4 plan, and
base sampling (host-issued steps and one hipGraph per step) against the real `DDIMSampler.sample` (hybrid_sample.npz).

Bounds: TOL_UNET / TOL_RMS of tests/test_unet_gpu.py carry over -- the concat adds no stored fp16 rounding to the residual path (the
first conv's input rows are rounded to fp16 once, as without it); TOL_BASE of tests/test_loops_gpu.py likewise (same model width, steps,
eta and guidance scale as the loop it was set on)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import FULL, REDUCED, golden, inp, relerr, state_dict_for  # noqa: E402
from test_loops_gpu import TOL_BASE  # noqa: E402
from test_unet_gpu import TOL_RMS, TOL_UNET, check  # noqa: E402

SHAPE = (8, 16, 16)
UNET = "lvdm.modules.networks.openaimodel3d.UNetModel"
# the in_channels = 4 `crossattn` plan of the reduced-width UNet at [1, 4, 8, 16, 16] with a 77-token context, read off the commit
# before hybrid conditioning: recorded launches and the plan's key
PARENT_STEPS = 741
PARENT_KEY = (1, 8, 16, 16, 77, torch.float32, 0, 0, False)


def _dm(in_channels, key):
    from moca_video_amd import DenoiseModel
    m = DenoiseModel({"target": UNET, "params": dict(REDUCED, in_channels=in_channels)}, conditioning_key=key)
    m.model.diffusion_model.load_state_dict(state_dict_for(m.model.diffusion_model, 11), strict=True)
    return m.cuda()


@pytest.fixture(scope="module")
def dm8():
    return _dm(8, "hybrid")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("Cpad,c0,k", [(8, 4, 4), (8, 0, 4), (8, 6, 2), (8, 5, 3), (16, 4, 4), (16, 8, 1), (16, 0, 9), (16, 12, 4)])
def test_scatter_kernel(dtype, Cpad, c0, k):
    """written columns are bit-equal to src.half() in channels-last order, every other column keeps its sentinel; odd HW"""
    from moca_video_amd import ops
    B, T, HW = 2, 3, 7 * 9
    g = torch.Generator().manual_seed(Cpad * 100 + c0 * 10 + k)
    src = (torch.randn(B, k, T, HW, generator=g) * 3).to(dtype).cuda()
    y = torch.full((B * T * HW, Cpad), -777.0, dtype=torch.float16, device="cuda")
    ops.ncthw_scatter(src, y, B=B, k=k, T=T, HW=HW, Cpad=Cpad, c0=c0)
    torch.cuda.synchronize()
    want = src.half().permute(0, 2, 3, 1).reshape(B * T * HW, k)
    assert torch.equal(y[:, c0:c0 + k], want)
    rest = torch.cat([y[:, :c0], y[:, c0 + k:]], 1)
    assert (rest == -777.0).all()


def _case(g, name, B, ks):
    x = inp(f"hybrid.{name}.x", (B, 4) + SHAPE).cuda()
    scale = float(g["concat_scale"])
    cc = [(inp(f"hybrid.{name}.cc{i}", (B, k) + SHAPE) * scale).cuda() for i, k in enumerate(ks)]
    ctx = inp(f"hybrid.{name}.ctx", (B, 77, 128)).cuda()
    return x, cc, ctx, torch.from_numpy(g[name + "__t"]).cuda()


@pytest.mark.parametrize("case,B,ks", [("a", 1, (4,)), ("b", 1, (4,)), ("c", 2, (2, 2)), ("d", 1, (4,))])
def test_hybrid_wrapper_vs_reference_golden(dm8, case, B, ks):
    """cases a-d of hybrid_wrapper.npz through DenoiseModel.apply_model with the reference's calling convention (a cond dict); d passes
    fps=[10] in the dict, which the hybrid branch drops (its golden is the reference's own output of that call)"""
    g = golden("hybrid_wrapper")
    x, cc, ctx, t = _case(g, "a" if case == "d" else case, B, ks)
    cond = {"c_concat": cc, "c_crossattn": [ctx]}
    if case == "d":
        cond["fps"] = torch.tensor([10]).cuda()
    ref = torch.from_numpy(g[case])
    for it in range(3):                          # eager pass, graph-capture pass, graph replay
        y = dm8.apply_model(x, t, cond)
        assert y.shape == ref.shape and y.dtype == x.dtype
        check(y.cpu(), ref, TOL_UNET, f"hybrid {case} pass {it}")


def test_hybrid_adm_mask_nine_channels_vs_reference_golden():
    """case e: in_channels = 9 (16-channel input rows), c_concat of 4 + 1 channels, key 'hybrid-adm-mask' with s= and mask="""
    g = golden("hybrid_wrapper")
    dm9 = _dm(9, "hybrid-adm-mask")
    x, cc, ctx, t = _case(g, "e", 1, (4, 1))
    ref = torch.from_numpy(g["e"])
    for it in range(3):
        y = dm9.apply_model(x, t, {"c_concat": cc, "c_crossattn": [ctx]}, s=torch.tensor([3]).cuda(), mask=torch.ones(1, 1, *SHAPE).cuda())
        check(y.cpu(), ref, TOL_UNET, f"hybrid e pass {it}")
    xc = torch.cat([x] + cc, 1)
    assert torch.equal(dm9.model.diffusion_model(xc, t, context=ctx), y)


def test_hybrid_equals_plain_forward_of_the_concat_bit_for_bit(dm8):
    """same kernels on the same operands from the first conv on: scattered pieces == ncthw_to_nhwc of torch.cat([x] + c_concat, 1)"""
    g = golden("hybrid_wrapper")
    unet = dm8.model.diffusion_model
    for name, B, ks in (("a", 1, (4,)), ("c", 2, (2, 2))):
        x, cc, ctx, t = _case(g, name, B, ks)
        xc = torch.cat([x] + cc, 1)
        for it in range(3):
            plain = unet(xc, t, context=ctx)
            hyb = dm8.apply_model(x, t, {"c_concat": cc, "c_crossattn": [ctx], "fps": torch.tensor([24]).cuda()})
            assert torch.equal(plain, hyb), f"case {name} pass {it}: {relerr(hyb.cpu(), plain.cpu()):.3e}"
        half = dm8.apply_model(x.half(), t, {"c_concat": [c.half() for c in cc], "c_crossattn": [ctx]})
        assert half.dtype == torch.float16 and torch.equal(half, unet(xc.half(), t, context=ctx))
    with pytest.raises(ValueError, match="in_channels=8"):
        dm8.apply_model(x, t, {"c_concat": cc[:1], "c_crossattn": [ctx]})


def test_four_channel_crossattn_plan_is_unchanged():
    """in_channels = 4, 'crossattn': the plan records what it recorded before hybrid conditioning existed, under the same key"""
    from moca_video_amd import DenoiseModel
    m = DenoiseModel({"target": UNET, "params": dict(REDUCED)})
    unet = m.model.diffusion_model
    unet.load_state_dict(state_dict_for(unet, 11), strict=True)
    m = m.cuda()
    x, ctx = inp("reduced.uniform.x", (1, 4) + SHAPE).cuda(), inp("reduced.uniform.ctx", (1, 77, 128)).cuda()
    m.apply_model(x, torch.tensor([500]).cuda(), {"c_crossattn": [ctx], "fps": 16})
    (key, plan), = unet._plans.items()
    assert key == PARENT_KEY[:6] + (x.device.index,) + PARENT_KEY[7:]
    assert len(plan.steps) == PARENT_STEPS
    assert plan.pieces is None and plan.x_rows is None and plan.steps[-1].func.__name__ == "nhwc_to_ncthw"
    assert sum(s.func.__name__ == "ncthw_to_nhwc" for s in plan.steps) == 1
    assert not any(s.func.__name__ == "ncthw_scatter" for s in plan.steps)


def _sample_inputs():
    g = golden("hybrid_sample")
    shape = [1, 4] + list(SHAPE)
    scale = float(g["concat_scale"])
    cond = {"c_concat": [(inp("hybrid.sample.cc0", shape) * scale).cuda()], "c_crossattn": [inp("hybrid.sample.ctx", (1, 77, 128)).cuda()],
            "fps": torch.tensor([10]).cuda()}
    return g, shape, cond, inp("hybrid.sample.uctx", (1, 77, 128)).cuda(), inp("hybrid.sample.x_T", shape).cuda(), \
        [inp(f"hybrid.sample.noise{i}", shape).cuda() for i in range(10)]


@pytest.mark.parametrize("use_graph", [False, True])
def test_hybrid_base_sampling_vs_reference_golden(dm8, use_graph):
    """base_ddim_sampling on the hybrid model: 10 steps, eta 1, CFG 12, use_scale, recorded x_T and noise -- against the real
    DDIMSampler.sample through the real apply_model; host-issued p_sample_ddim and one hipGraph per step (fifo_graph.BaseEngine)"""
    from moca_video_amd.fifo import base_ddim_sampling
    from moca_video_amd.fifo_graph import BaseEngine
    g, shape, cond, uctx, x_T, noises = _sample_inputs()
    uc = dict(cond, c_crossattn=[uctx])
    assert BaseEngine.supported(dm8, x_T, cond, uc, 12.0)
    _, sampler, samples = base_ddim_sampling(dm8, cond, shape, 10, 1.0, 12.0, uc_emb=uctx, x_T=x_T, noises=noises, use_graph=use_graph)
    e = relerr(samples.cpu(), g["samples"])
    print(f"[parity] hybrid base sampling use_graph={use_graph}: rel err {e:.3e}")
    assert e < TOL_BASE, f"samples rel err {e:.3e}"


def test_hybrid_step_graph_is_deterministic_and_rewrites_c_concat(dm8):
    """graph path: the same seed and noises give bit-identical latents; reset() with another c_concat moves the result by more than
    TOL_BASE (the constant columns of the input rows are rewritten), and back again restores it bit for bit"""
    from moca_video_amd.fifo_graph import BaseEngine
    from moca_video_amd.sampler import DDIMSampler
    g, shape, cond, uctx, x_T, noises = _sample_inputs()
    uc = dict(cond, c_crossattn=[uctx])
    s = DDIMSampler(dm8)
    s.make_schedule(10, ddim_eta=1.0, verbose=False)
    eng = BaseEngine(dm8, s, x_T, cond, uc, 12.0, seed=5)

    def run(c, u, fixed=True):
        eng.reset(x_T, c, u, 5)
        for i in range(10):
            eng.step(noise=noises[i] if fixed else None)
        return eng.latents()
    a, b = run(cond, uc), run(cond, uc)
    assert torch.equal(a, b) and torch.isfinite(a).all()
    assert relerr(a.cpu(), g["samples"]) < TOL_BASE
    assert eng.plan.graph is not None
    other = [inp("hybrid.sample.cc_other", shape).cuda() * float(g["concat_scale"])]
    c2 = dict(cond, c_concat=other)
    d = run(c2, dict(uc, c_concat=other))
    moved = relerr(d.cpu(), a.cpu())
    print(f"[parity] another c_concat moves the sampled latents by {moved:.3e}")
    assert moved > TOL_BASE
    assert torch.equal(run(cond, uc), a)
    r1, r2 = run(cond, uc, fixed=False), run(cond, uc, fixed=False)      # the device noise stream
    assert torch.equal(r1, r2)
    eng.close()


def test_hybrid_full_width_vs_reference_golden():
    """the YAML's UNet with in_channels = 8, one 'hybrid' call at [1, 8, 16, 40, 64]"""
    from moca_video_amd import DenoiseModel
    g = golden("unet_full_hybrid")
    m = DenoiseModel({"target": UNET, "params": dict(FULL, in_channels=8)}, conditioning_key="hybrid")
    m.model.diffusion_model.load_state_dict(state_dict_for(m.model.diffusion_model, 11), strict=True)
    m = m.cuda()
    shp = (16, 40, 64)
    x, cc = inp("full_hybrid.x", (1, 4) + shp).cuda(), inp("full_hybrid.cc0", (1, 4) + shp).cuda()
    ctx = inp("full_hybrid.ctx", (1, 77, 1024)).cuda()
    ref = torch.from_numpy(g["hybrid"])
    for it in range(3):
        y = m.apply_model(x, torch.from_numpy(g["hybrid__t"]).cuda(), {"c_concat": [cc], "c_crossattn": [ctx]})
        check(y.cpu(), ref, TOL_UNET, f"full-width hybrid pass {it}")
