"""GPU: causal temporal attention (both forms: the standalone kernel and the MOCA_EP_TATTN epilogue) against an fp32 torch restatement
of attention.py:92-114 with the mask of :101-105; the temporal cross-attention (`temporal_selfatt_only=False`); blocks and UNets of
both variants against goldens of the REAL reference (tools/make_golden_temporal_variants.py) under the bounds tests/test_unet_gpu.py
applies to the plain model -- the variants cross the same number of fp16 roundings per path; the shared-prefix forward, one
BaseEngine step and a FifoEngine.set_context switch on such models."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import FULL, REDUCED, golden, inp, relerr, state_dict_for  # noqa: E402
from test_unet_gpu import TOL_BLOCK, TOL_UNET, check  # noqa: E402
import temporal_variants_ref as R  # noqa: E402

TOL16 = 3e-3                   # tests/test_kernels_gpu.py: one fp16-output kernel against fp32 torch on the same fp16 operands


def _kcheck(got, ref, what):
    e = relerr(got, ref)
    print(f"[kernel] {what}: max-norm rel err {e:.2e}")
    assert torch.isfinite(got.float()).all(), what
    assert e < TOL16, f"{what}: {e:.3e}"


def _perturb_later_frames(t2d, B, T, HW, t0):
    """a copy of the [B*T*HW][C] rows with the rows of every frame > t0 replaced"""
    out = t2d.clone().view(B, T, HW, -1)
    out[:, t0 + 1:] = (out[:, t0 + 1:].float() * -1.7 + 0.9).to(out.dtype)
    return out.view_as(t2d)


# ---------------------------------------------------------------- standalone kernel
@pytest.mark.parametrize("B,T,HW,heads", R.STANDALONE + [(2, 16, 21, 3)])
def test_causal_temporal_attention_kernel(B, T, HW, heads):
    from moca_video_amd import ops
    C = heads * 64
    qkv = R.standalone_operands(B, T, HW, heads)

    def run(x):
        out = torch.full((B * T * HW, C), float("nan"), dtype=torch.float16, device="cuda")
        ops.temporal_attention_causal(x[:, :C], x[:, C:2 * C], x[:, 2 * C:], out, B=B, T=T, HW=HW, heads=heads, ld_qkv=3 * C, ldo=C,
                                      scale=R.SCALE)
        return out
    out = run(qkv)
    _kcheck(out, R.standalone_ref(qkv, B, T, HW, heads, True), f"causal temporal attention {(B, T, HW, heads)}")
    assert relerr(out, R.standalone_ref(qkv, B, T, HW, heads, False)) > 20 * TOL16, "the mask is not visible on these operands"
    assert torch.equal(run(qkv), out) and torch.equal(run(qkv), out), "replays must be bit-identical"
    # frame 0 attends to itself only: its output IS v of frame 0
    v0 = qkv.view(B, T, HW, 3, C)[:, 0, :, 2]
    assert torch.equal(out.view(B, T, HW, C)[:, 0], v0)
    for t0 in sorted({0, T // 3, T - 2}):                         # output rows of frames <= t0 do not depend on later frames, bit for bit
        got = run(_perturb_later_frames(qkv, B, T, HW, t0)).view(B, T, HW, C)
        assert torch.equal(got[:, :t0 + 1], out.view(B, T, HW, C)[:, :t0 + 1]), f"frames <= {t0} moved with later frames"
        assert not torch.equal(got[:, t0 + 1:], out.view(B, T, HW, C)[:, t0 + 1:])


# ---------------------------------------------------------------- fused epilogue
@pytest.mark.parametrize("B,HW,heads,K,fold", R.FUSED)
def test_causal_fused_projection_and_attention(B, HW, heads, K, fold):
    from moca_video_amd import ops
    x, ws, gb = R.fused_operands(B, HW, heads, K, fold)
    out = R.fused_run(ops, x, ws, gb, B, HW, heads, True)
    C = heads * 64
    _kcheck(out, R.fused_ref(x, ws, gb, B, HW, heads, True), f"fused causal {(B, HW, heads, K, fold)}")
    assert relerr(out, R.fused_ref(x, ws, gb, B, HW, heads, False)) > 20 * TOL16, "the mask is not visible on these operands"
    for _ in range(2):
        assert torch.equal(R.fused_run(ops, x, ws, gb, B, HW, heads, True), out), "replays must be bit-identical"
    for t0 in (0, 6, 14):
        got = R.fused_run(ops, _perturb_later_frames(x, B, 16, HW, t0), ws, gb, B, HW, heads, True).view(B, 16, HW, C)
        assert torch.equal(got[:, :t0 + 1], out.view(B, 16, HW, C)[:, :t0 + 1]), f"frames <= {t0} moved with later frames"
    # the two forms agree to fp16 noise on the same projection (the standalone kernel reads q|k|v rounded to fp16, as the epilogue does)
    if not fold:
        qkv = torch.cat([(x.float() @ w.float().t()).half() for w in ws], dim=1).contiguous()
        o2 = torch.empty_like(out)
        ops.temporal_attention_causal(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], o2, B=B, T=16, HW=HW, heads=heads, ld_qkv=3 * C, ldo=C,
                                      scale=R.SCALE)
        assert relerr(out, o2) < TOL16


def test_non_causal_entries_keep_the_parent_commits_bits():
    """moca_temporal_attention_f16 and the non-causal MOCA_EP_TATTN launch: sha256 of the output equals the one recorded with the
    parent commit's library on the same operands (tools/record_parent_fixtures.py --sha re-records it).  The cases are those of
    tests/test_kernels_gpu.py::test_temporal_attention / ::test_gemm_temporal_attention_fused -- same shapes, same operand
    construction (x * 1.5 + 0.3 with the fold, weights scaled by K ** -0.5, LayerNorm weights 1 + 0.3 z) -- but NOT that file's operand
    bits: its rnd() seeds from a call counter, so its values depend on which tests ran before, and a hash needs operands that are
    the same bits in every process.  They come from moca_video_amd.weightgen by name instead (tests/temporal_variants_ref.py)."""
    from moca_video_amd import ops
    g = golden("temporal_attention_parent_sha")
    want = {str(n): str(s) for n, s in zip(g["names"], g["sha256"])}
    assert len(want) == len(R.STANDALONE) + len(R.FUSED)
    for B, T, HW, heads in R.STANDALONE:
        C = heads * 64
        qkv = R.standalone_operands(B, T, HW, heads)
        out = torch.zeros(B * T * HW, C, dtype=torch.float16, device="cuda")
        ops.temporal_attention(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], out, B=B, T=T, HW=HW, heads=heads, ld_qkv=3 * C, ldo=C,
                               scale=R.SCALE)
        _kcheck(out, R.standalone_ref(qkv, B, T, HW, heads, False), f"temporal attention {(B, T, HW, heads)}")
        assert R.sha(out) == want[f"standalone.{B}.{T}.{HW}.{heads}"], (B, T, HW, heads)
    for B, HW, heads, K, fold in R.FUSED:
        x, ws, gb = R.fused_operands(B, HW, heads, K, fold)
        out = R.fused_run(ops, x, ws, gb, B, HW, heads, False)
        _kcheck(out, R.fused_ref(x, ws, gb, B, HW, heads, False), f"fused {(B, HW, heads, K, fold)}")
        assert R.sha(out) == want[f"fused.{B}.{HW}.{heads}.{K}.{int(fold)}"], (B, HW, heads, K, fold)


# ---------------------------------------------------------------- blocks against goldens of the real reference blocks
def _filled(block, seed):
    block.load_state_dict(state_dict_for(block, seed), strict=True)
    return block.cuda()


def _run_block(run, x5, **kw):
    b, c, t, h, w = x5.shape
    y = run(x5.permute(0, 2, 1, 3, 4).reshape(b * t, c, h, w).cuda(), **kw).cpu()
    return y.reshape(b, t, c, h, w).permute(0, 2, 1, 3, 4)


def test_block_causal_temporal_transformer_vs_reference_golden():
    """a: T = 16, HW = 20 -- the fused launch; b: T = 8 = temporal_length, HW = 15 -- the standalone kernel"""
    from moca_video_amd.blockplan import BlockRunner
    from moca_video_amd.unet import _TemporalTransformer
    g = golden("block_temporal_causal")
    for name, shape, fused in (("a", (2, 128, 16, 4, 5), True), ("b", (1, 128, 8, 3, 5), False)):
        B, _, T, H, W = shape
        blk = _filled(_TemporalTransformer(128, 2, 64, 1, True, causal_attention=True, temporal_length=T), 21)
        run = BlockRunner(blk, B=B, T=T, H=H, W=W)
        names = [s.func.__name__ for s in run.plan.steps]
        assert ("temporal_attention_causal" not in names) == fused and "temporal_attention" not in names
        assert sum(1 for s in run.plan.steps if len(s.keywords.get("tattn") or ()) > 3) == (2 if fused else 0)
        for it in range(3):
            check(_run_block(run, inp(f"ttc.{name}.x", shape)), torch.from_numpy(g[name]), TOL_BLOCK, f"causal temporal transformer {name} pass {it}")


def test_block_temporal_cross_transformer_vs_reference_golden():
    """one context PER VIDEO (case a: two videos, two different 77-token contexts; case b: 154 tokens)"""
    from moca_video_amd.blockplan import BlockRunner
    from moca_video_amd.unet import _TemporalTransformer
    g = golden("block_temporal_cross")
    for name, shape, L in (("a", (2, 128, 4, 4, 4), 77), ("b", (1, 128, 8, 4, 4), 154)):
        B, _, T, H, W = shape
        blk = _filled(_TemporalTransformer(128, 2, 64, 1, True, context_dim=96, only_self_att=False, temporal_length=16), 22)
        run = BlockRunner(blk, B=B, T=T, H=H, W=W, L=L, context_dim=96)
        ctx = inp(f"ttx.{name}.ctx", (B, L, 96)).cuda()
        for it in range(3):
            check(_run_block(run, inp(f"ttx.{name}.x", shape), context=ctx), torch.from_numpy(g[name]), TOL_BLOCK,
                  f"temporal cross transformer {name} pass {it}")
        if B == 2:                                               # the contexts are per video: swapping them is visible
            assert relerr(_run_block(run, inp(f"ttx.{name}.x", shape), context=ctx.flip(0)), g[name]) > 20 * TOL_BLOCK


# ---------------------------------------------------------------- reduced-width UNets against goldens of the real reference UNet
def _reduced(**kw):
    from moca_video_amd import UNetModel
    m = UNetModel(**dict(REDUCED, **kw))
    m.load_state_dict(state_dict_for(m, 11), strict=True)
    return m.cuda()


@pytest.fixture(scope="module")
def causal_model():
    return _reduced(use_causal_attention=True)


@pytest.fixture(scope="module")
def cross_model():
    return _reduced(temporal_selfatt_only=False)


@pytest.fixture(scope="module")
def both_model():
    return _reduced(temporal_selfatt_only=False, use_causal_attention=True)


def _golden_case(model, case, shape):
    g = golden("unet_reduced_tvariants")
    L = int(g[case + "__L"])
    x = inp(f"tv.{case}.x", shape).cuda()
    ctx = inp(f"tv.{case}.ctx", (shape[0], L, 128)).cuda()
    t = torch.from_numpy(g[case + "__t"]).cuda()
    fps = torch.from_numpy(np.atleast_1d(g[case + "__fps"])).cuda()
    ref = torch.from_numpy(g[case])
    for it in range(3):                                          # eager pass, graph-capture pass, graph replay
        y = model(x, t, context=ctx, fps=fps)
        assert y.shape == ref.shape
        check(y.cpu(), ref, TOL_UNET, f"{case} pass {it}")
    assert any(p.graph is not None for p in model._plans.values()), "hipGraph replay path was not taken"


@pytest.mark.parametrize("case", ["causal", "causal_fifo"])
def test_unet_reduced_causal_vs_reference_golden(causal_model, case):
    _golden_case(causal_model, case, (1, 4, 16, 8, 40))
    names = [s.func.__name__ for p in causal_model._plans.values() for s in p.steps]
    assert "temporal_attention_causal" in names and "temporal_attention" not in names       # HW = 5 at the lowest level


@pytest.mark.parametrize("case,shape", [("cross", (2, 4, 4, 16, 16)), ("cross154", (1, 4, 16, 32, 32))])
def test_unet_reduced_temporal_cross_vs_reference_golden(cross_model, case, shape):
    _golden_case(cross_model, case, shape)


def test_unet_reduced_both_flags_vs_reference_golden(both_model):
    """T = 8 on a model built with temporal_length = 16: the cross branch never uses the mask (attention.py:362-363), nothing is refused"""
    _golden_case(both_model, "both", (1, 4, 8, 32, 32))


def test_causal_unet_refuses_another_frame_count(causal_model):
    x = inp("tv.bad.x", (1, 4, 8, 16, 16)).cuda()
    with pytest.raises(ValueError, match="temporal_length = 16"):
        causal_model(x, torch.tensor([500]).cuda(), context=inp("tv.bad.ctx", (1, 77, 128)).cuda())


def test_unet_full_width_causal_vs_reference_golden():
    """the YAML's UNet with use_causal_attention at the headline shape [1,4,16,40,64] (per-frame timesteps, 77 tokens): the fused causal
    launch at the 320- / 640- / 1280-channel levels"""
    from moca_video_amd import UNetModel
    g = golden("unet_full_causal")
    m = UNetModel(**dict(FULL, use_causal_attention=True))
    m.load_state_dict(state_dict_for(m, 11), strict=True)
    m = m.cuda()
    x = inp("full_causal.fifo16.x", (1, 4, 16, 40, 64)).cuda()
    ctx = inp("full_causal.fifo16.ctx", (1, 77, 1024)).cuda()
    t = torch.from_numpy(g["fifo16__t"]).cuda()
    fps = torch.from_numpy(np.atleast_1d(g["fifo16__fps"])).cuda()
    runs = [m(x, t, context=ctx, fps=fps) for _ in range(3)]
    check(runs[0].cpu(), torch.from_numpy(g["fifo16"]), TOL_UNET, "full-width causal fifo16")
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[1], runs[2]), "replays must be bit-identical"
    plan = next(iter(m._plans.values()))
    assert sum(1 for s in plan.steps if len(s.keywords.get("tattn") or ()) > 3) > 0
    m._invalidate()


# ---------------------------------------------------------------- integration
@pytest.mark.parametrize("which", ["causal", "cross"])
def test_shared_prefix_equals_separate_forwards(causal_model, cross_model, which):
    """forward_segments(shared_x=True): on the temporal-cross model the prefix ends at init_attn's attn2"""
    model, shape = (causal_model, (2, 4, 16, 8, 40)) if which == "causal" else (cross_model, (2, 4, 4, 16, 16))
    x = inp("tv.sp.x", shape).cuda()
    c154, c77 = inp("tv.sp.c154", (2, 154, 128)).cuda(), inp("tv.sp.c77", (2, 77, 128)).cuda()
    fps = torch.tensor([10, 24]).cuda()
    t = torch.tensor([981, 20]).cuda()
    ref = torch.cat([model(x, t, context=c154, fps=fps), model(x, t, context=c77, fps=fps)], 0)
    for it in range(3):
        out = model.forward_segments(x, t, [c154, c77], fps=[fps, fps], shared_x=True)
        assert out.shape == ref.shape
        e = relerr(out, ref)
        print(f"[shared prefix] {which} pass {it}: {e:.2e}")
        assert e < TOL_UNET, f"shared prefix ({which}), pass {it}: {e:.2e}"


def _dm(**kw):
    from moca_video_amd import DenoiseModel
    dm = DenoiseModel({"target": "lvdm.modules.networks.openaimodel3d.UNetModel", "params": dict(REDUCED, **kw)})
    m = dm.model.diffusion_model
    m.load_state_dict(state_dict_for(m, 11), strict=True)
    return dm.cuda()


@pytest.mark.parametrize("flags,shape", [(dict(use_causal_attention=True), (1, 4, 16, 8, 40)),
                                         (dict(temporal_selfatt_only=False, use_causal_attention=True), (1, 4, 8, 32, 32))])
def test_base_engine_step_equals_host_issued_two_call_path(flags, shape):
    """one hipGraph per DDIM step (fifo_graph.BaseEngine: shared-prefix UNet, guidance, update) against DDIMSampler.p_sample_ddim issued
    from the host on the same latents and noise -- on a causal model (the step graph replays the causal launches of both forms:
    HW = 320 / 80 / 20 fused, HW = 5 standalone) and on a model with BOTH flags (temporal cross-attention; the mask reaches nothing).
    Bound: the two paths run the UNet on other batch shapes (other tilings), each within TOL_UNET of the exact eps; guidance 12
    multiplies the difference of the two branches, as in tests/test_unet_gpu.py::test_shared_cfg_prefix (4 x TOL_UNET)."""
    from moca_video_amd.fifo_graph import BaseEngine
    from moca_video_amd.sampler import DDIMSampler
    dm = _dm(**flags)
    s = DDIMSampler(dm)
    s.make_schedule(6, ddim_eta=1.0, verbose=False)
    x0 = inp("tv.be.x", shape).cuda()
    fps = torch.tensor([10]).cuda()
    cond = {"c_crossattn": [inp("tv.be.c", (1, 77, 128)).cuda()], "fps": fps}
    uc = {"c_crossattn": [inp("tv.be.uc", (1, 77, 128)).cuda()], "fps": fps}
    assert BaseEngine.supported(dm, x0, cond, uc, 12.0)
    eng = BaseEngine(dm, s, x0, cond, uc, 12.0, seed=5, keep_pred_x0=True)
    x, worst = x0.clone(), 0.0
    for i in range(3):
        index = 5 - i
        n = inp(f"tv.be.n{i}", x.shape).cuda()
        ts = torch.full((1,), int(s.ddim_timesteps[index]), device="cuda", dtype=torch.long)
        x_ref, p_ref = s.p_sample_ddim(x, cond, ts, index=index, unconditional_guidance_scale=12.0, unconditional_conditioning=uc, noise=n)
        eng.step(noise=n)
        got = eng.latents()
        worst = max(worst, relerr(got.cpu(), x_ref.cpu()), relerr(eng.last_pred_x0().cpu(), p_ref.cpu()))
        x = got
    print(f"[base engine] {sorted(flags)}: worst rel err against p_sample_ddim {worst:.2e}")
    assert worst < 4 * TOL_UNET
    unet_steps = [st for st in eng.plan.steps if hasattr(st, "func") and hasattr(st, "keywords")]     # (the engine adds steps of its own)
    causal_only = "temporal_selfatt_only" not in flags
    assert any(st.func.__name__ == "temporal_attention_causal" for st in unet_steps) == causal_only
    assert any(len(st.keywords.get("tattn") or ()) > 3 for st in unet_steps) == causal_only
    eng.close()


def test_fifo_engine_set_context_on_a_temporal_cross_model():
    """the temporal attn2 K|V columns live in the one up-front context GEMM of the recorded iteration, so a prompt switch is a copy into
    the plan's context rows: an engine built with prompt A and switched to B before its first iteration computes, bit for bit, what a
    fresh engine built with B computes (eager, capture, replay); a later switch keeps the captured graph"""
    from moca_video_amd.fifo import prepare_latents
    from moca_video_amd.fifo_graph import FifoEngine
    from moca_video_amd.sampler import DDIMSampler
    dm = _dm(temporal_selfatt_only=False)
    args = types.SimpleNamespace(num_inference_steps=16, video_length=8, lookahead_denoising=True, num_partitions=2, new_video_length=10)
    s = DDIMSampler(dm)
    s.make_schedule(16, ddim_eta=1.0, verbose=False)
    prep = [inp(f"tv.fe.prep{i}", (1, 4, 1, 32, 32)) for i in range(20)]
    lat = prepare_latents(args, None, s, initial_latents=inp("tv.fe.z", (1, 4, 8, 32, 32)).cuda(), noises=prep)
    ca, cb, ucx = (inp(f"tv.fe.{k}", (1, 77, 128)).cuda() for k in ("ca", "cb", "uc"))
    fps = torch.tensor([10]).cuda()
    noises = [[inp(f"tv.fe.n{i}.{w}", (1, 4, 8, 32, 32)).cuda() for w in range(4)] for i in range(4)]
    shifts = [inp(f"tv.fe.s{i}", (1, 4, 32, 32)).cuda() for i in range(4)]

    def engine(c):
        return FifoEngine(args, dm, s, {"c_crossattn": [c], "fps": fps}, {"c_crossattn": [ucx], "fps": fps}, 12.0, lat.clone())
    sw, fresh, other = engine(ca), engine(cb), engine(ca)
    sw.set_context(cb)
    for i in range(3):
        for e in (sw, fresh, other):
            e.step(noise=noises[i], shift_noise=shifts[i])
        assert torch.equal(sw.latents(), fresh.latents()), f"iteration {i}: switched engine != fresh engine with the new context"
        assert not torch.equal(sw.latents(), other.latents())
    graph = sw.plan.graph.value
    assert graph and not sw.plan.graph_failed
    sw.set_context(ca)                                            # a switch behind the capture: same graph, prompt A's result from here on
    fresh.set_context(ca)
    sw.step(noise=noises[3], shift_noise=shifts[3])
    fresh.step(noise=noises[3], shift_noise=shifts[3])
    assert sw.plan.graph.value == graph and torch.equal(sw.latents(), fresh.latents())
    for e in (sw, fresh, other):
        e.close()
