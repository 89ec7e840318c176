"""GPU: temporal attention over 17 .. 32 frames.  The kernel (moca_temporal_attention_long_f16) against the fp32 torch restatement of
attention.py:92-114 with the mask of :101-105 on the same fp16 operands; its continuity with the 16-frame kernel; blocks and UNets
past 16 frames against goldens of the REAL reference (tools/make_golden_long_frames.py) under the bounds tests/test_unet_gpu.py
applies at 16 frames -- the number of fp16 roundings on a path does not depend on T; the GroupNorm statistics of a 32-frame group;
the shared-prefix forward, one BaseEngine step sequence and DDIMSampler.sample on a 24-frame clip."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import FULL, REDUCED, golden, inp, relerr, state_dict_for  # noqa: E402
from test_unet_gpu import TOL_BLOCK, TOL_UNET, check  # noqa: E402
import long_frames_ref as R  # noqa: E402

TOL16 = 3e-3                   # tests/test_kernels_gpu.py: one fp16-output kernel against fp32 torch on the same fp16 operands
GUARD = 64                     # rows behind the output that no launch may touch


def _kcheck(got, ref, what):
    e = relerr(got, ref)
    print(f"[kernel] {what}: max-norm rel err {e:.2e}")
    assert torch.isfinite(got.float()).all(), what
    assert e < TOL16, f"{what}: {e:.3e}"
    return e


def _run(q, k, v, B, T, HW, heads, causal, ld_qkv, ldo):
    """one launch into a NaN-filled [rows + GUARD][ldo] buffer: returns the [rows][C] result after checking that every element of it
    was written and nothing else (the pad columns of a row, the guard rows behind the last one) was"""
    from moca_video_amd import ops
    C, rows = heads * 64, B * T * HW
    buf = torch.full((rows + GUARD, ldo), float("nan"), dtype=torch.float16, device="cuda")
    ops.temporal_attention_long(q, k, v, buf, B=B, T=T, HW=HW, heads=heads, ld_qkv=ld_qkv, ldo=ldo, scale=R.SCALE, causal=causal)
    torch.cuda.synchronize()
    assert not torch.isnan(buf[:rows, :C]).any(), "an output element was not written (or is NaN)"
    assert torch.isnan(buf[rows:]).all() and torch.isnan(buf[:rows, C:]).all(), "a store landed outside the output"
    return buf[:rows, :C].clone()


def _perturb_later_frames(t2d, B, T, HW, t0):
    """a copy of the [B*T*HW][C] rows with the rows of every frame > t0 replaced"""
    out = t2d.clone().view(B, T, HW, -1)
    out[:, t0 + 1:] = (out[:, t0 + 1:].float() * -1.7 + 0.9).to(out.dtype)
    return out.view_as(t2d)


# ---------------------------------------------------------------- the kernel
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("B,T,HW,heads", R.KERNEL)
def test_long_temporal_attention_kernel(B, T, HW, heads, causal):
    C = heads * 64
    qkv = R.operands(B, T, HW, heads)
    run = lambda x: _run(x[:, :C], x[:, C:2 * C], x[:, 2 * C:], B, T, HW, heads, causal, 3 * C, C)
    ref = {c: R.reference(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], B, T, HW, heads, c) for c in (False, True)}
    out = run(qkv)
    _kcheck(out, ref[causal], f"long temporal attention {(B, T, HW, heads)} causal={causal}")
    assert relerr(ref[True], ref[False]) > 20 * TOL16, "the mask is not visible on these operands"
    assert torch.equal(run(qkv), out) and torch.equal(run(qkv), out), "replays must be bit-identical"
    if not causal:
        return
    o4 = out.view(B, T, HW, C)
    # frame 0 attends to itself only: its output IS v of frame 0
    assert torch.equal(o4[:, 0], qkv.view(B, T, HW, 3, C)[:, 0, :, 2])
    for t0 in sorted({0, T // 3, 16, T - 2}):                     # output rows of frames <= t0 do not depend on later frames, bit for bit
        got = run(_perturb_later_frames(qkv, B, T, HW, t0)).view(B, T, HW, C)
        assert torch.equal(got[:, :t0 + 1], o4[:, :t0 + 1]), f"frames <= {t0} moved with later frames"
        assert t0 == T - 1 or not torch.equal(got[:, t0 + 1:], o4[:, t0 + 1:])      # (T = 17: t0 = 16 is the last frame, nothing is perturbed)


@pytest.mark.parametrize("causal", [False, True])
def test_long_kernel_strides_and_column_offsets(causal):
    """ld_qkv = 3C + 8, ldo = C + 4; q, k, v are views of ONE buffer that start at columns 8, 8 + C, 8 + 2C"""
    B, T, HW, heads = R.STRIDED
    C, rows = heads * 64, B * T * HW
    buf = torch.full((rows, 3 * C + 8), 777.0, dtype=torch.float16, device="cuda")
    buf[:, 8:] = R.operands(B, T, HW, heads, tag="s")
    q, k, v = buf[:, 8:8 + C], buf[:, 8 + C:8 + 2 * C], buf[:, 8 + 2 * C:]
    out = _run(q, k, v, B, T, HW, heads, causal, 3 * C + 8, C + 4)
    _kcheck(out, R.reference(q, k, v, B, T, HW, heads, causal), f"long temporal attention, strided {R.STRIDED} causal={causal}")


@pytest.mark.parametrize("causal", [False, True])
def test_continuity_with_the_16_frame_kernel(causal):
    """a 16-frame problem padded to 17 frames by one frame that no query of frames 0 .. 15 can reach computes, on those frames, what
    the 16-frame kernel computes.  Causal: the mask hides frame 16 from every earlier frame.  Non-causal: frame 16's key is made
    unreachable through a large negative k -- every q of the case carries +3 in its first coordinate, k of frame 16 is -300 there and
    zero elsewhere, so every score against it is -900 * SCALE = -112 while the other scores stay within a few units: its probability
    is < exp(-100), zero in the fp16 P (and below 1e-6 in the fp32 reference, asserted)."""
    from moca_video_amd import ops
    B, HW, heads = 2, 21, 3
    C = heads * 64
    x16 = R.operands(B, 16, HW, heads, tag="c").view(B, 16, HW, 3, heads, 64).clone()
    extra = R.operands(B, 1, HW, heads, tag="cx").view(B, 1, HW, 3, heads, 64).clone()
    if not causal:
        x16[:, :, :, 0, :, 0] = 3.0                              # q: a common positive first coordinate
        extra[:, :, :, 1] = 0.0
        extra[:, :, :, 1, :, 0] = -300.0                         # k of frame 16: q . k = -900 for every query of frames 0 .. 15
    x17 = torch.cat([x16, extra], dim=1).reshape(B * 17 * HW, 3 * C).contiguous()
    x16 = x16.reshape(B * 16 * HW, 3 * C).contiguous()
    got17 = _run(x17[:, :C], x17[:, C:2 * C], x17[:, 2 * C:], B, 17, HW, heads, causal, 3 * C, C).view(B, 17, HW, C)[:, :16]
    old = torch.full((B * 16 * HW, C), float("nan"), dtype=torch.float16, device="cuda")
    fn = ops.temporal_attention_causal if causal else ops.temporal_attention
    fn(x16[:, :C], x16[:, C:2 * C], x16[:, 2 * C:], old, B=B, T=16, HW=HW, heads=heads, ld_qkv=3 * C, ldo=C, scale=R.SCALE)
    ref17 = R.reference(x17[:, :C], x17[:, C:2 * C], x17[:, 2 * C:], B, 17, HW, heads, causal).view(B, 17, HW, C)[:, :16]
    ref16 = R.reference(x16[:, :C], x16[:, C:2 * C], x16[:, 2 * C:], B, 16, HW, heads, causal).view(B, 16, HW, C)
    assert relerr(ref17, ref16) < 1e-6, "the padding frame is reachable in the reference itself"
    _kcheck(got17, old.view(B, 16, HW, C), f"frames 0..15 of T = 17 against the 16-frame kernel, causal={causal}")
    _kcheck(got17, ref17, f"frames 0..15 of T = 17 against the padded fp32 reference, causal={causal}")


# ---------------------------------------------------------------- blocks against goldens of the real reference blocks
def _filled(block, seed):
    block.load_state_dict(state_dict_for(block, seed), strict=True)
    return block.cuda()


def _run_block(run, x5, **kw):
    b, c, t, h, w = x5.shape
    y = run(x5.permute(0, 2, 1, 3, 4).reshape(b * t, c, h, w).cuda(), **kw).cpu()
    return y.reshape(b, t, -1, h, w).permute(0, 2, 1, 3, 4)


@pytest.mark.parametrize("name,shape,causal,tl,seed", [("tt24", (1, 128, 24, 3, 5), False, 16, 31), ("ttc32", (2, 128, 32, 4, 5), True, 32, 32)])
def test_block_temporal_transformer_vs_reference_golden(name, shape, causal, tl, seed):
    from moca_video_amd.blockplan import BlockRunner
    from moca_video_amd.unet import _TemporalTransformer
    B, _, T, H, W = shape
    kw = dict(causal_attention=True) if causal else {}
    run = BlockRunner(_filled(_TemporalTransformer(128, 2, 64, 1, True, temporal_length=tl, **kw), seed), B=B, T=T, H=H, W=W)
    long_steps = [s for s in run.plan.steps if s.func.__name__ == "temporal_attention_long"]
    assert len(long_steps) == 2 and all(s.keywords["causal"] is causal for s in long_steps)
    ref = torch.from_numpy(golden("block_long_frames")[name])
    for it in range(3):
        check(_run_block(run, inp(f"lf.{name}.x", shape)), ref, TOL_BLOCK, f"temporal transformer {name} pass {it}")


def test_block_resblock_24_frames_vs_reference_golden():
    """ResBlock + TemporalConvBlock on 24 frames: the temporal-conv GEMM (tconv = (C, 24, HW)) and the 5-D GroupNorms
    (frames_per_stat = 24) on their own"""
    from moca_video_amd.blockplan import BlockRunner
    from moca_video_amd.unet import _ResBlock
    run = BlockRunner(_filled(_ResBlock(64, 256, 128, True), 33), B=1, T=24, H=3, W=5)
    x, emb = inp("lf.rb24.x", (24, 64, 3, 5)).cuda(), inp("lf.rb24.emb", (24, 256)).cuda()
    ref = golden("block_long_frames")["rb24"]
    for it in range(3):
        check(run(x, emb=emb).cpu(), ref, TOL_BLOCK, f"resblock, 24 frames, pass {it}")


# ---------------------------------------------------------------- reduced-width UNets against goldens of the real reference UNet
def _reduced(**kw):
    from moca_video_amd import UNetModel
    m = UNetModel(**dict(REDUCED, **kw))
    m.load_state_dict(state_dict_for(m, 11), strict=True)
    return m.cuda()


@pytest.fixture(scope="module")
def plain_model():
    return _reduced()


def _golden_case(model, g, case, shape):
    L = int(g[case + "__L"])
    x = inp(f"lf.{case}.x", shape).cuda()
    ctx = inp(f"lf.{case}.ctx", (shape[0], L, 128)).cuda()
    t = torch.from_numpy(g[case + "__t"]).cuda()
    fps = torch.from_numpy(np.atleast_1d(g[case + "__fps"])).cuda()
    ref = torch.from_numpy(g[case])
    for it in range(3):                                          # eager pass, graph-capture pass, graph replay
        y = model(x, t, context=ctx, fps=fps)
        assert y.shape == ref.shape
        check(y.cpu(), ref, TOL_UNET, f"{case} pass {it}")
    assert any(p.graph is not None for p in model._plans.values()), "hipGraph replay path was not taken"
    names = [s.func.__name__ for p in model._plans.values() for s in p.steps]
    assert "temporal_attention_long" in names


@pytest.mark.parametrize("case,shape", [("plain24", (1, 4, 24, 16, 16)), ("fifo32", (1, 4, 32, 8, 40))])
def test_unet_reduced_vs_reference_golden(plain_model, case, shape):
    _golden_case(plain_model, golden("unet_reduced_long_frames"), case, shape)


def test_unet_reduced_causal24_vs_reference_golden():
    _golden_case(_reduced(use_causal_attention=True, temporal_length=24), golden("unet_reduced_long_frames"), "causal24", (1, 4, 24, 8, 8))


def test_unet_reduced_cross32_vs_reference_golden():
    """temporal_selfatt_only=False at 32 frames: every level's h*w (2048, 512, 128, 32) is a multiple of 32"""
    _golden_case(_reduced(temporal_selfatt_only=False), golden("unet_reduced_long_frames_cross32"), "cross32", (1, 4, 32, 32, 64))


def test_unet_full_width_32_frames_vs_reference_golden():
    """the YAML's UNet at [1,4,32,40,64] (per-frame timesteps, 77 tokens): the shape with the largest GroupNorm statistics groups of a
    T <= 32 forward at 40 x 64 latents (32 x 2560 rows x 10 channels)"""
    from moca_video_amd import UNetModel
    g = golden("unet_full_long_frames")
    ref = torch.cat([torch.from_numpy(g["fifo32"]), torch.from_numpy(golden("unet_full_long_frames_b")["fifo32"])], dim=2)
    m = UNetModel(**FULL)
    m.load_state_dict(state_dict_for(m, 11), strict=True)
    m = m.cuda()
    x = inp("full_long.fifo32.x", (1, 4, 32, 40, 64)).cuda()
    ctx = inp("full_long.fifo32.ctx", (1, 77, 1024)).cuda()
    t = torch.from_numpy(g["fifo32__t"]).cuda()
    fps = torch.from_numpy(np.atleast_1d(g["fifo32__fps"])).cuda()
    runs = [m(x, t, context=ctx, fps=fps) for _ in range(3)]
    check(runs[0].cpu(), ref, TOL_UNET, "full-width fifo32")
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[1], runs[2]), "replays must be bit-identical"
    plan = next(iter(m._plans.values()))
    assert sum(1 for s in plan.steps if s.func.__name__ == "temporal_attention_long") == 2 * 17
    m._invalidate()


# ---------------------------------------------------------------- GroupNorm statistics of a 32-frame group
@pytest.mark.parametrize("knob", [2, 0])
def test_groupnorm_statistics_of_a_32_frame_group(knob):
    """MOCA_EP_GSTAT -> groupnorm_gstat as the UNet takes them for a 5-D GroupNorm at the 320-channel level of a 32-frame clip
    (frames_per_stat = 32, HW = 2560, C = 320: 819 200 values and up to 2^10 partials per group), on the weight-stationary (2) and the
    tiled (0) 320 -> 320 linear, at rms 1e3 and 4e3 against a two-pass float64 GroupNorm of the tensor the kernel read (bound: TOL16 of
    tests/test_groupnorm_gpu.py).  Beyond the range of csrc/common.h -- a group's sum of squares >= 2^49 = 5.6e14, here 819 200 values
    of magnitude 3e4 = 7.4e14 -- the statistics read back as NaN: every output element is NaN, none a finite wrong number."""
    from moca_video_amd import lib as L, ops
    from test_groupnorm_gpu import check as gcheck, gn_ref
    old = L.set_tuning(L.MOCA_TUNE_GEMM_WS, knob)
    try:
        Fr, HW, C, fps, eps = 32, 2560, 320, 32, 1e-5
        M = Fr * HW
        a = R.host("gn.a", M, C).half().cuda()
        pw = ops.pack_linear(R.host("gn.w", C, C, scale=C ** -0.5).half().cuda(), (R.host("gn.b", C) * 0.1).cuda())
        g, be = (R.host("gn.g", C) * 0.2 + 1.0).cuda(), (R.host("gn.be", C) * 0.2).cuda()
        noise = R.host("gn.res", M, C).cuda()
        for rms in (1e3, 4e3):
            res = (noise * rms).half()
            gst = torch.zeros(64, dtype=torch.int64, device="cuda")
            out = torch.empty(M, C, dtype=torch.float16, device="cuda")
            ops.gemm(a, pw, out, M=M, residual=res, gstat=(gst, fps * HW))
            y = torch.empty_like(out)
            ops.groupnorm_gstat(out, y, g, be, gst, F=Fr, HW=HW, Cn=C, frames_per_stat=fps, eps=eps, silu=True)
            got_rms = out.float().pow(2).mean().sqrt().item()
            assert 0.9 * rms < got_rms < 1.1 * rms
            gcheck(y, gn_ref(out, g, be, 1, eps, True), f"groupnorm_gstat over 32 frames (ws={knob}) rms={rms:g}")
        res = (torch.sign(noise) * 3e4).half()
        gst = torch.zeros(64, dtype=torch.int64, device="cuda")
        out = torch.empty(M, C, dtype=torch.float16, device="cuda")
        ops.gemm(a, pw, out, M=M, residual=res, gstat=(gst, fps * HW))
        assert torch.isfinite(out).all()
        y = torch.zeros_like(out)
        ops.groupnorm_gstat(out, y, g, be, gst, F=Fr, HW=HW, Cn=C, frames_per_stat=fps, eps=eps, silu=True)
        assert torch.isnan(y).all(), "statistics beyond the fixed-point range must read back as NaN"
    finally:
        L.set_tuning(L.MOCA_TUNE_GEMM_WS, old)


# ---------------------------------------------------------------- integration at reduced width
def test_shared_prefix_equals_separate_forwards_at_24_frames(plain_model):
    x = inp("lf.sp.x", (2, 4, 24, 16, 16)).cuda()
    c154, c77 = inp("lf.sp.c154", (2, 154, 128)).cuda(), inp("lf.sp.c77", (2, 77, 128)).cuda()
    fps = torch.tensor([10, 24]).cuda()
    t = torch.tensor([981, 20]).cuda()
    ref = torch.cat([plain_model(x, t, context=c154, fps=fps), plain_model(x, t, context=c77, fps=fps)], 0)
    for it in range(3):
        out = plain_model.forward_segments(x, t, [c154, c77], fps=[fps, fps], shared_x=True)
        assert out.shape == ref.shape
        e = relerr(out, ref)
        print(f"[shared prefix] 24 frames, pass {it}: {e:.2e}")
        assert e < TOL_UNET, f"shared prefix, pass {it}: {e:.2e}"


def _dm():
    from moca_video_amd import DenoiseModel
    dm = DenoiseModel({"target": "lvdm.modules.networks.openaimodel3d.UNetModel", "params": dict(REDUCED)})
    m = dm.model.diffusion_model
    m.load_state_dict(state_dict_for(m, 11), strict=True)
    return dm.cuda()


def test_base_engine_step_equals_host_issued_two_call_path_at_24_frames():
    """one hipGraph per DDIM step (fifo_graph.BaseEngine) against DDIMSampler.p_sample_ddim issued from the host on the same latents
    and noise.  Bound and reasoning of tests/test_temporal_variants_gpu.py::test_base_engine_step_equals_host_issued_two_call_path:
    the two paths run the UNet on other batch shapes, each within TOL_UNET of the exact eps; guidance 12 multiplies the difference of
    the two branches (4 x TOL_UNET)."""
    from moca_video_amd.fifo_graph import BaseEngine
    from moca_video_amd.sampler import DDIMSampler
    dm = _dm()
    s = DDIMSampler(dm)
    s.make_schedule(6, ddim_eta=1.0, verbose=False)
    shape = (1, 4, 24, 16, 16)
    x0 = inp("lf.be.x", shape).cuda()
    fps = torch.tensor([10]).cuda()
    cond = {"c_crossattn": [inp("lf.be.c", (1, 77, 128)).cuda()], "fps": fps}
    uc = {"c_crossattn": [inp("lf.be.uc", (1, 77, 128)).cuda()], "fps": fps}
    assert BaseEngine.supported(dm, x0, cond, uc, 12.0)
    eng = BaseEngine(dm, s, x0, cond, uc, 12.0, seed=5, keep_pred_x0=True)
    x, worst = x0.clone(), 0.0
    for i in range(3):
        index = 5 - i
        n = inp(f"lf.be.n{i}", shape).cuda()
        ts = torch.full((1,), int(s.ddim_timesteps[index]), device="cuda", dtype=torch.long)
        x_ref, p_ref = s.p_sample_ddim(x, cond, ts, index=index, unconditional_guidance_scale=12.0, unconditional_conditioning=uc, noise=n)
        eng.step(noise=n)
        got = eng.latents()
        worst = max(worst, relerr(got.cpu(), x_ref.cpu()), relerr(eng.last_pred_x0().cpu(), p_ref.cpu()))
        x = got
    print(f"[base engine] 24 frames: worst rel err against p_sample_ddim {worst:.2e}")
    assert worst < 4 * TOL_UNET
    assert any(getattr(getattr(st, "func", None), "__name__", "") == "temporal_attention_long" for st in eng.plan.steps)
    eng.close()


def test_ddim_sample_24_frames_on_the_one_graph_path():
    from moca_video_amd.sampler import DDIMSampler
    dm = _dm()
    s = DDIMSampler(dm)
    shape = (1, 4, 24, 16, 16)
    fps = torch.tensor([10]).cuda()
    cond = {"c_crossattn": [inp("lf.ds.c", (1, 77, 128)).cuda()], "fps": fps}
    uc = {"c_crossattn": [inp("lf.ds.uc", (1, 77, 128)).cuda()], "fps": fps}
    out = s.sample(S=4, batch_size=1, shape=shape[1:], conditioning=cond, eta=1.0, x_T=inp("lf.ds.x_T", shape).cuda(),
                   unconditional_guidance_scale=12.0, unconditional_conditioning=uc,
                   noises=[inp(f"lf.ds.n{i}", shape).cuda() for i in range(4)])[0]
    assert tuple(out.shape) == shape and torch.isfinite(out).all()
    assert s._base_engine is not None and s._base_engine[1].plan.graph is not None, "the one-graph path was not taken"
    s.release()


def test_wrappers_return_their_output_buffer():
    """ops.temporal_attention, ops.temporal_attention_causal and ops.temporal_attention_long return `out`, as every wrapper of ops does"""
    from moca_video_amd import ops
    for fn, T, kw in ((ops.temporal_attention, 16, {}), (ops.temporal_attention_causal, 16, {}),
                      (ops.temporal_attention_long, 17, {}), (ops.temporal_attention_long, 17, dict(causal=True))):
        qkv = R.operands(1, T, 3, 1, tag="w")
        out = torch.empty(T * 3, 64, dtype=torch.float16, device="cuda")
        assert fn(qkv[:, :64], qkv[:, 64:128], qkv[:, 128:], out, B=1, T=T, HW=3, heads=1, ld_qkv=192, ldo=64, scale=R.SCALE, **kw) is out
