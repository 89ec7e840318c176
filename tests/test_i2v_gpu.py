"""GPU: image cross-attention (use_image_attention=True; attention.py:82-87,117-124).

The fused kernel (moca_attention_ip_f16) against an fp32 torch restatement of the two-softmax formula, under the bound of
test_kernels_gpu.py::test_attention (3e-3 max-norm); the image-attention UNet against goldens of the REAL reference
(tools/make_golden_i2v.py) under the whole-UNet bounds of test_unet_gpu.py (max-norm 4.5e-3 and relative RMS 4e-3: the fused kernel
rounds the same one P per key to fp16 as the text-only kernel, so the per-store error model of that file is unchanged); and the plan's
routing: a <= 77-token context takes the text-only kernel bit for bit, the shared-CFG-prefix plan equals separate forwards."""
import pytest
import torch

from helpers import REDUCED, golden, inp, relerr, state_dict_for

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL16 = 3e-3
TOL_UNET, TOL_RMS = 4.5e-3, 4e-3


def rnd(*shape, scale=1.0, gen=[None]):
    if gen[0] is None:
        gen[0] = torch.Generator(device="cpu").manual_seed(1234)
    return (torch.randn(*shape, generator=gen[0]) * scale).half().to(DEV)


def rmserr(got, ref):
    got, ref = torch.as_tensor(got).float(), torch.as_tensor(ref).float()
    return ((got - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt().clamp_min(1e-20)).item()


def check_unet(got, ref, what):
    e, r = relerr(got, ref), rmserr(got, ref)
    print(f"[parity] {what}: max-norm rel err {e:.2e}, rel rms {r:.2e}")
    assert e < TOL_UNET and r < TOL_RMS, f"{what}: max-norm {e:.3e} (tol {TOL_UNET}), rms {r:.3e} (tol {TOL_RMS})"


def ip_ref(q, k, v, ki, vi, heads, kv_div, scale, ip_scale):
    """attention.py:92-124 in fp32: two separate softmaxes, out + ip_scale * out_ip"""
    def sm(qq, kk, vv):
        Bq, Nq, C = qq.shape
        sp = lambda t: t.float().reshape(t.shape[0], t.shape[1], heads, 64).permute(0, 2, 1, 3)
        kh, vh = sp(kk).repeat_interleave(kv_div, 0), sp(vv).repeat_interleave(kv_div, 0)
        p = torch.softmax(sp(qq) @ kh.transpose(-1, -2) * scale, -1)
        return (p @ vh).permute(0, 2, 1, 3).reshape(Bq, Nq, C)
    return sm(q, k, v) + ip_scale * sm(q, ki, vi)


def run_ip(Bq, heads, Nq, Nt, Ni, kv_div, ip_scale):
    from moca_video_amd import ops
    C = heads * 64
    Bk = Bq // kv_div
    q = rnd(Bq, Nq, C)
    kv, kvi = rnd(Bk, Nt, 2 * C), rnd(Bk, Ni, 2 * C)         # interleaved K|V rows (strided operands, as the plan passes them)
    k, v, ki, vi = kv[..., :C], kv[..., C:], kvi[..., :C], kvi[..., C:]
    out = torch.full((Bq, Nq, C), float("nan"), dtype=torch.float16, device=DEV)
    ops.attention_ip(q, k, v, ki, vi, out, Bq=Bq, heads=heads, Nq=Nq, Nt=Nt, Ni=Ni, ldq=C, ldk=2 * C, ldv=2 * C, ldk_ip=2 * C,
                     ldv_ip=2 * C, ldo=C, kv_div=kv_div, scale=0.125, ip_scale=ip_scale)
    return out, (q, k, v, ki, vi)


@pytest.mark.parametrize("Bq,heads,Nq,Nt,Ni,kv_div,ip_scale", [
    (2, 5, 2560, 77, 16, 1, 1.0),
    (4, 10, 640, 77, 4, 2, 1.0),
    (3, 20, 160, 1, 1, 1, 1.0),
    (2, 5, 1000, 80, 16, 2, 0.7),          # the largest tile; Nq tail (1000 = 7 x 128 + 104)
    (16, 5, 200, 77, 16, 8, 2.5),          # kv_div 8 (frames of a video), Nq tail
    (1, 5, 33, 40, 9, 1, 1.0),
])
def test_attention_ip_vs_two_softmax_formula(Bq, heads, Nq, Nt, Ni, kv_div, ip_scale):
    out, (q, k, v, ki, vi) = run_ip(Bq, heads, Nq, Nt, Ni, kv_div, ip_scale)
    ref = ip_ref(q, k, v, ki, vi, heads, kv_div, 0.125, ip_scale)
    e = relerr(out, ref)
    print(f"[parity] attention_ip Nt={Nt} Ni={Ni}: {e:.2e}")
    assert torch.isfinite(out).all() and e < TOL16, e


def test_attention_ip_segment_maxima_differ():
    """the image logits sit > 20 above the text logits (in natural-log units): one shared maximum would underflow every text P"""
    from moca_video_amd import ops
    Bq, heads, Nq, Nt, Ni, C = 2, 5, 300, 77, 16, 320
    q, kv, kvi = rnd(Bq, Nq, C), rnd(Bq, Nt, 2 * C), rnd(Bq, Ni, 2 * C)
    q = q.clone(); q[..., 0::64] = 1.0
    kvi = kvi.clone(); kvi[..., 0:C:64] = 30.0 / 0.125                # + 30 on every image logit of every head
    k, v, ki, vi = kv[..., :C], kv[..., C:], kvi[..., :C], kvi[..., C:]
    ref = ip_ref(q, k, v, ki, vi, heads, 1, 0.125, 1.0)
    out = torch.empty(Bq, Nq, C, dtype=torch.float16, device=DEV)
    ops.attention_ip(q, k, v, ki, vi, out, Bq=Bq, heads=heads, Nq=Nq, Nt=Nt, Ni=Ni, ldq=C, ldk=2 * C, ldv=2 * C, ldk_ip=2 * C,
                     ldv_ip=2 * C, ldo=C, kv_div=1, scale=0.125, ip_scale=1.0)
    sp = lambda t: t.float().reshape(Bq, -1, heads, 64).permute(0, 2, 1, 3)
    gap = ((sp(q) @ sp(ki).transpose(-1, -2)).amax(-1) - (sp(q) @ sp(k).transpose(-1, -2)).amax(-1)) * 0.125
    assert gap.min().item() > 20
    e = relerr(out, ref)
    print(f"[parity] attention_ip, segment maxima {gap.min().item():.1f} apart: {e:.2e}")
    assert e < TOL16, e


@pytest.mark.parametrize("Bq,heads,Nq,Nt,kv_div", [(2, 5, 2560, 77, 1), (16, 10, 300, 77, 8), (3, 20, 129, 50, 1)])
def test_attention_ip_without_image_tokens_is_attention(Bq, heads, Nq, Nt, kv_div):
    from moca_video_amd import ops
    C = heads * 64
    q, kv = rnd(Bq, Nq, C), rnd(Bq // kv_div, Nt, 2 * C)
    a = torch.empty(Bq, Nq, C, dtype=torch.float16, device=DEV)
    b = torch.empty_like(a)
    ops.attention(q, kv[..., :C], kv[..., C:], a, Bq=Bq, heads=heads, Nq=Nq, Nk=Nt, ldq=C, ldk=2 * C, ldv=2 * C, ldo=C, kv_div=kv_div,
                  scale=0.125)
    ops.attention_ip(q, kv[..., :C], kv[..., C:], kv[..., :C], kv[..., C:], b, Bq=Bq, heads=heads, Nq=Nq, Nt=Nt, Ni=0, ldq=C, ldk=2 * C,
                     ldv=2 * C, ldk_ip=2 * C, ldv_ip=2 * C, ldo=C, kv_div=kv_div, scale=0.125, ip_scale=1.0)
    assert torch.equal(a, b)


# ---- the image-attention UNet ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def i2v_model():
    from moca_video_amd import UNetModel
    m = UNetModel(**dict(REDUCED, use_image_attention=True))
    m.load_state_dict(state_dict_for(m, 11), strict=True)
    return m.cuda()


@pytest.mark.parametrize("case,B", [("uniform93", 1), ("frames81", 1), ("batch2", 2)])
def test_unet_i2v_vs_reference_golden(i2v_model, case, B):
    g = golden("unet_reduced_i2v")
    L = int(g[case + "__L"])
    x = inp(f"reduced_i2v.{case}.x", (B, 4, 8, 16, 16)).cuda()
    ctx = inp(f"reduced_i2v.{case}.ctx", (B, L, 128)).cuda()
    t = torch.from_numpy(g[case + "__t"]).cuda()
    fps = g[case + "__fps"]
    fps = int(fps) if fps.ndim == 0 else torch.from_numpy(fps).cuda()
    ref = torch.from_numpy(g[case])
    for it in range(3):          # eager, capture, replay
        y = i2v_model(x, t, context=ctx, fps=fps)
        check_unet(y.cpu(), ref, f"i2v {case} pass {it}")
    # the image tokens matter: without them the output moves far outside the bound
    y77 = i2v_model(x, t, context=ctx[:, :77].contiguous(), fps=fps)
    assert relerr(y77.cpu(), ref) > 20 * TOL_UNET


def test_unet_i2v_77_tokens_equals_t2v_path(i2v_model):
    """a 77-token context: the reference's image slice is empty, the plan launches the text-only kernel -- bit for bit the t2v UNet with
    the same text weights"""
    from moca_video_amd import UNetModel
    t2v = UNetModel(**REDUCED)
    sd = {k: v for k, v in state_dict_for(i2v_model, 11).items() if "_ip" not in k}
    t2v.load_state_dict(sd, strict=True)
    t2v = t2v.cuda()
    x = inp("i2v77.x", (2, 4, 8, 16, 16)).cuda()
    ctx = inp("i2v77.ctx", (2, 77, 128)).cuda()
    t, fps = torch.tensor([981, 20]).cuda(), torch.tensor([10, 24]).cuda()
    assert torch.equal(i2v_model(x, t, context=ctx, fps=fps), t2v(x, t, context=ctx, fps=fps))


def test_unet_i2v_shared_cfg_prefix_equals_separate_forwards(i2v_model):
    """the two CFG branches with 93-token contexts (and a 93 / 81 pair, and a 93 / 77 pair: image rows in one branch only) as one
    shared-prefix forward against one plain forward per branch"""
    x = inp("i2vsp.x", (2, 4, 8, 16, 16)).cuda()
    fps = torch.tensor([10, 24]).cuda()
    t = torch.tensor([981, 20]).cuda()
    c93, u93 = inp("i2vsp.c93", (2, 93, 128)).cuda(), inp("i2vsp.u93", (2, 93, 128)).cuda()
    u81, u77 = inp("i2vsp.u81", (2, 81, 128)).cuda(), inp("i2vsp.u77", (2, 77, 128)).cuda()
    for uc in (u93, u81, u77):
        ref = torch.cat([i2v_model(x, t, context=c93, fps=fps), i2v_model(x, t, context=uc, fps=fps)], 0)
        for it in range(3):
            out = i2v_model.forward_segments(x, t, [c93, uc], fps=[fps, fps], shared_x=True)
            assert out.shape == ref.shape
            e = relerr(out, ref)
            assert e < TOL_UNET, f"shared prefix {uc.shape[1]} tokens, pass {it}: {e:.2e}"
    # plain multi-segment batch: per-segment launches on their own text / image rows
    xs = torch.cat([x, x.flip(0)], 0)
    out = i2v_model.forward_segments(xs, torch.cat([t, t]), [c93, u81], fps=torch.cat([fps, fps]))
    ref = torch.cat([i2v_model(x, t, context=c93, fps=fps), i2v_model(x.flip(0), t, context=u81, fps=fps)], 0)
    assert relerr(out, ref) < TOL_UNET


def test_unet_i2v_refuses_a_longer_context(i2v_model):
    x = inp("i2v77.x", (1, 4, 8, 16, 16)).cuda()
    with pytest.raises(ValueError, match="longer than 93"):
        i2v_model(x, torch.tensor([500]).cuda(), context=torch.zeros(1, 94, 128, device=DEV))


def test_packed_operands_carry_the_image_projection(i2v_model):
    """dist.broadcast_packed sends what the recorded launches read: the packed to_{k,v}_ip weights are part of it"""
    from moca_video_amd import dist as mdist
    x = inp("i2v77.x", (1, 4, 8, 16, 16)).cuda()
    i2v_model(x, torch.tensor([500]).cuda(), context=inp("i2vop.ctx", (1, 93, 128)).cuda())
    ops_ = mdist.packed_operands(i2v_model._packed, list(i2v_model._plans.values()))
    ip = i2v_model._packed["ctx_kv_ip_all"]
    assert any(t.data_ptr() == ip.w.data_ptr() for t in ops_)


# ---- projectors, full width, the model shell and the sampling loops ------------------------------------------------------------
# projector bounds: one fp16 rounding per stored activation (~30 stores on the Resampler's longest path: sqrt(30) x 2.8e-4 = 1.5e-3
# predicted relative rms).  Observed on an MI355X: Resampler max-norm 1.44e-3 / rms 1.14e-3 (zero image 1.24e-3 / 1.14e-3),
# ImageProjModel 5.97e-4 / 4.11e-4.  Bounds = 1.5 x the largest observed value
TOL_PROJ, TOL_PROJ_RMS = 2.2e-3, 1.7e-3


def _resampler():
    from moca_video_amd import Resampler
    m = Resampler(dim=1024, depth=4, dim_head=64, heads=12, num_queries=16, embedding_dim=1280, output_dim=1024, ff_mult=4)
    m.load_state_dict(state_dict_for(m, 21), strict=True)
    return m.cuda()


def _improj():
    from moca_video_amd import ImageProjModel
    m = ImageProjModel(clip_extra_context_tokens=4, cross_attention_dim=1024, clip_embeddings_dim=1024)
    m.load_state_dict(state_dict_for(m, 22), strict=True)
    return m.cuda()


def _check_proj(got, ref, what):
    e, r = relerr(got, ref), rmserr(got, ref)
    print(f"[parity] {what}: max-norm rel err {e:.2e}, rel rms {r:.2e}")
    assert got.dtype == torch.float32 and got.shape == tuple(ref.shape)
    assert e < TOL_PROJ and r < TOL_PROJ_RMS, f"{what}: max-norm {e:.3e}, rms {r:.3e}"


def test_projectors_vs_reference_golden():
    from i2v_standin import StandInImageEmbedder
    g = golden("image_proj")
    res, imp = _resampler(), _improj()
    _check_proj(res(inp("i2v.resampler.x", (2, 257, 1280)).cuda()).cpu(), torch.from_numpy(g["resampler"]), "Resampler")
    _check_proj(imp(inp("i2v.improj.x", (2, 1024)).cuda()).cpu(), torch.from_numpy(g["improj"]), "ImageProjModel")
    zero = torch.zeros(2, 3, 224, 224, device=DEV)
    _check_proj(res(StandInImageEmbedder(True).cuda()(zero)).cpu(), torch.from_numpy(g["resampler_zero_image"]), "Resampler, zero image")
    _check_proj(imp(StandInImageEmbedder(False).cuda()(zero)).cpu(), torch.from_numpy(g["improj_zero_image"]), "ImageProjModel, zero image")


def test_unet_full_width_i2v_vs_reference_golden():
    from helpers import FULL
    from moca_video_amd import UNetModel
    g = golden("unet_full_i2v")
    m = UNetModel(**dict(FULL, use_image_attention=True))
    m.load_state_dict(state_dict_for(m, 11), strict=True)
    m = m.cuda()
    x = inp("full_i2v.ctx93.x", (1, 4, 16, 40, 64)).cuda()
    ctx = inp("full_i2v.ctx93.ctx", (1, 93, 1024)).cuda()
    fps = torch.from_numpy(g["ctx93__fps"]).cuda()
    for it in range(2):
        y = m(x, torch.from_numpy(g["ctx93__t"]).cuda(), context=ctx, fps=fps)
        check_unet(y.cpu(), torch.from_numpy(g["ctx93"]), f"full-width i2v pass {it}")
    del m
    torch.cuda.empty_cache()


def _lvd(finegrained=True):
    from i2v_standin import StandInImageEmbedder
    from moca_video_amd import LatentVisualDiffusion
    m = LatentVisualDiffusion({"target": "lvdm.modules.encoders.condition.FrozenOpenCLIPImageEmbedderV2"}, finegrained,
                              unet_config={"target": "lvdm.modules.networks.openaimodel3d.UNetModel",
                                           "params": dict(REDUCED, context_dim=1024, use_image_attention=True)})
    assert m.embedder is None                   # the vision tower's target does not import here: the seam
    with pytest.raises(RuntimeError, match="no image embedder"):
        m.get_image_embeds(torch.zeros(1, 3, 224, 224))
    unet = m.model.diffusion_model
    unet.load_state_dict(state_dict_for(unet, 11), strict=True)
    proj = m.image_proj_model
    proj.load_state_dict(state_dict_for(proj, 21 if finegrained else 22), strict=True)
    m.embedder = StandInImageEmbedder(finegrained)
    return m.cuda()


def test_base_ddim_sampling_appends_the_zero_image_embedding():
    """funcs.py:207-210: with an `embedder`, the unconditional context is cat(uc_emb, get_image_embeds(zero image)) -- 77 + 16 tokens.
    The image tokens of the zero image match the reference projector's (golden); the whole sampling run equals the same run on a
    model without an embedder that is handed that 93-token unconditional context (bit for bit: same plan, same draws)."""
    from moca_video_amd import DenoiseModel
    from moca_video_amd.fifo import base_ddim_sampling
    lvd = _lvd(True)
    zero_emb = lvd.get_image_embeds(torch.zeros(1, 3, 224, 224, device=DEV))
    _check_proj(zero_emb.cpu(), torch.from_numpy(golden("image_proj")["resampler_zero_image"][:1]), "get_image_embeds(zero image)")
    shape = [1, 4, 8, 16, 16]
    c93, u77 = inp("i2v.loop.c93", (1, 93, 1024)).cuda(), inp("i2v.loop.u77", (1, 77, 1024)).cuda()
    x_T = inp("i2v.loop.xT", shape).cuda()
    noises = [inp(f"i2v.loop.noise{i}", shape).cuda() for i in range(3)]
    cond = {"c_crossattn": [c93], "fps": torch.tensor([10]).cuda()}
    _, _, got = base_ddim_sampling(lvd, cond, shape, 3, 1.0, 12.0, uc_emb=u77, x_T=x_T, noises=noises)
    plain = DenoiseModel({"target": "lvdm.modules.networks.openaimodel3d.UNetModel", "params": dict(REDUCED, context_dim=1024)})
    plain.model = lvd.model                      # the same UNet; no `embedder` attribute (the t2v shape of the model)
    plain = plain.cuda()
    assert not hasattr(plain, "embedder")
    _, _, ref = base_ddim_sampling(plain, cond, shape, 3, 1.0, 12.0, uc_emb=torch.cat([u77, zero_emb], 1), x_T=x_T, noises=noises)
    assert torch.isfinite(got).all() and torch.equal(got, ref)


def test_base_step_graph_equals_p_sample_ddim_with_image_tokens():
    """fifo_graph.BaseEngine (one hipGraph per DDIM step) with 93-token contexts on both guidance branches against
    DDIMSampler.p_sample_ddim step by step, same noise; same seed -> same latents, next seed -> different"""
    from moca_video_amd.fifo_graph import BaseEngine
    from moca_video_amd.sampler import DDIMSampler
    lvd = _lvd(True)
    s = DDIMSampler(lvd)
    s.make_schedule(6, ddim_eta=1.0, verbose=False)
    g = torch.Generator(device="cuda").manual_seed(3)
    x0 = torch.randn(2, 4, 8, 16, 16, device="cuda", generator=g)
    fps = torch.tensor([10, 12]).cuda()
    img = lvd.get_image_embeds(torch.rand(2, 3, 224, 224, device=DEV, generator=g))
    uimg = lvd.get_image_embeds(torch.zeros(2, 3, 224, 224, device=DEV))
    cond = {"c_crossattn": [torch.cat([inp("i2v.be.c", (2, 77, 1024)).cuda(), img], 1)], "fps": fps}
    uc = {"c_crossattn": [torch.cat([inp("i2v.be.u", (2, 77, 1024)).cuda(), uimg], 1)], "fps": fps}
    assert cond["c_crossattn"][0].shape[1] == 93 and BaseEngine.supported(lvd, x0, cond, uc, 12.0)
    eng = BaseEngine(lvd, s, x0, cond, uc, 12.0, seed=5, keep_pred_x0=True)
    x = x0.clone()
    worst = 0.0
    for i in range(6):
        index = 5 - i
        n = torch.randn(x.shape, device="cuda", generator=g)
        ts = torch.full((2,), int(s.ddim_timesteps[index]), device="cuda", dtype=torch.long)
        x_ref, p_ref = s.p_sample_ddim(x, cond, ts, index=index, unconditional_guidance_scale=12.0, unconditional_conditioning=uc, noise=n)
        eng.step(noise=n)
        got = eng.latents()
        worst = max(worst, relerr(got.cpu(), x_ref.cpu()), relerr(eng.last_pred_x0().cpu(), p_ref.cpu()))
        x = got
    assert worst < 1e-5, f"graph step vs p_sample_ddim {worst:.3e}"

    def run(seed):
        eng.reset(x0, cond, uc, seed)
        for _ in range(6):
            eng.step()
        return eng.latents()
    a, b, c = run(9), run(9), run(10)
    assert torch.equal(a, b) and torch.isfinite(a).all()
    assert not torch.equal(a, c)
    assert eng.plan.graph is not None
    eng.close()
